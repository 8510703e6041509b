// ledger.cpp — the qp_ledger_* entry points (qpgpu.h): Wormhole transfers
// settled after verification.  Each nullifier is admitted once, only storage
// roots the ledger knows are accepted, the padding proof's inputs are set
// aside, and the amounts are credited to the exit accounts.  With a context the
// raw public inputs are uploaded and screened, packed, inserted and credited on
// the device (ledger.hip); without one the same semantics run on the host
// (ql::HostLedger).  Both paths state the checks once, in ledger_table.h.
// The log commitment (commit_log, receipts, entries_at, roots_at and the
// receipt check: ledger_log.h) is the ledger's LogCommit (log_commit.h), brought
// up to date on demand; a cast does not touch it, and the tree is allocated by
// the first commit only.  The nullifier-set commitment (commit_set, set_proofs:
// nullifier_set.h) is the ledger's SetCommit (set_commit.h) over the credited
// entries, rebuilt on demand only.  The payout claims commitment (commit_claims,
// claims: claims.h) is the ledger's ClaimsCommit (claims_commit.h) over the rows
// of one payout round, keyed by the range and built on demand only.  The refusals worded alike for the ledger and the
// ballot box are handle_common.h's; what is stated here is the ledger's own.
// qp_ledger_restore reopens a ledger from a published log through the audit's
// passes (ledger_audit.h; on the device qla::audit_screen_insert_resolve,
// shared with qp_ledger_log_audit) over the new ledger's own buffers;
// qp_ledger_payouts_between is a payout round over the ledger's log
// (ledger_rounds.h; the device launches are ledger_rounds.cpp's).
#include "../../include/qpgpu.h"
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "acc_tree.h"
#include "claims_commit.h"
#include "ctx.h"
#include "handle_common.h"
#include "ledger_audit.h"
#include "ledger_audit_device.h"
#include "ledger_kernels.h"
#include "ledger_log.h"
#include "ledger_rounds.h"
#include "ledger_table.h"
#include "log_commit.h"
#include "set_commit.h"
#include "verifier.h"

static_assert(sizeof(qp_transfer_result) == sizeof(ql::Result) && sizeof(ql::Result) == 24 &&
                  sizeof(qpk::LedgerResult) == 24,
              "qp_transfer_result layout");
static_assert(QP_TRANSFER_CREDITED == ql::CREDITED && QP_TRANSFER_PROOF_REJECTED == ql::PROOF_REJECTED &&
                  QP_TRANSFER_MALFORMED == ql::MALFORMED && QP_TRANSFER_PADDING == ql::PADDING &&
                  QP_TRANSFER_BAD_AMOUNT == ql::BAD_AMOUNT && QP_TRANSFER_UNKNOWN_ROOT == ql::UNKNOWN_ROOT &&
                  QP_TRANSFER_DOUBLE_SPEND == ql::DOUBLE_SPEND,
              "qp_transfer_status and ledger_table.h differ");
static_assert(QP_RECEIPT_OK == ql::RECEIPT_OK && QP_RECEIPT_SHAPE == ql::RECEIPT_SHAPE &&
                  QP_RECEIPT_ROOT == ql::RECEIPT_ROOT && QP_RECEIPT_NON_CANONICAL == ql::RECEIPT_NON_CANONICAL &&
                  QP_RECEIPT_NULL == ql::RECEIPT_NULL,
              "qp_receipt_status and ledger_log.h differ");

using namespace qph;
using qla::LedgerTables;

namespace {
// entries per launch of the lookups and gathers (their buffers hold this many)
constexpr uint32_t QUERY_BATCH = 8192;
}  // namespace

struct qp_ledger : ql::Words {
  static constexpr int BROKEN = QP_ERR_HIP;  // what a broken invariant returns (the box: QP_ERR_STATE)
  qp_ctx *ctx = nullptr;                     // null: the host path
  std::string err;
  bool dead = false;  // a device step failed part-way, or the defensive error word was set: no further calls
  ql::Screen screen;
  uint64_t cast = 0;
  ql::Packed pk;  // the host path's batch in flight
  ql::HostLedger host;
  // ---- device path
  uint64_t capacity = 0, count = 0, credited = 0, accounts = 0;  // credited / accounts: the device counters as of the last cast
  LedgerTables t;
  DevBuf d_roots, d_ctr, d_audit;
  uint32_t batch_room = 0;                          // transfers the per-batch buffers hold
  DevBuf d_pis, d_ver, d_res, d_blk, d_pos, d_stay;  // per batch: inputs, verdicts, results, block counts (+ total), pos, stay
  DevBuf d_pblk, d_payee;                           // the payees' block counts (+ total); the payees
  uint64_t payee_room = 0;                          // log entries d_pblk / d_payee are sized for
  bool payee_valid = false;                         // d_payee lists the accounts of the log as it is
  DevBuf d_q, d_qsum, d_qaux;                       // per lookup / gather batch (QUERY_BATCH entries)
  TimingEvents<3> ev;                               // upload start, upload end, resolve end of the last cast
  float ms[2] = {0, 0};
  LogCommit<ql::HostLog> lc;               // the log commitment, both paths
  SetCommit sc;                            // the nullifier-set commitment, both paths
  ClaimsCommit cc;                         // the payout claims commitment of one range, both paths
  DevBuf d_gacc, d_gnum, d_gamt, d_gflag;  // per entries_at batch, beside d_q (the seqs) and d_qsum (the nullifiers)
  uint64_t admitted() const { return ctx ? count : host.count(); }
  uint64_t cap() const { return ctx ? capacity : host.capacity; }
  uint64_t ncredited() const { return ctx ? credited : host.credited; }
  uint64_t naccounts() const { return ctx ? accounts : host.accounts(); }
};

namespace {
// why the last qp_ledger_new (restore, log_audit, log_payouts_between) on this thread was refused
thread_local HandlelessError g_new_err;

int refuse_new(qp_ctx *c, const std::string &why) {
  g_new_err.set(c, "qp_ledger_new: " + why);
  return QP_ERR_ARG;
}
}  // namespace

void qla::set_ledgerless_error(qp_ctx *c, const std::string &why) { g_new_err.set(c, why); }

namespace {
// the defensive error word after a launch (copied by the caller, stream synchronised)
int error_word(qp_ledger *l, const char *fn, uint32_t err) {
  if (!err) return QP_OK;
  return refuse(l, l->BROKEN,
                std::string(fn) +
                    (err & 1 ? ": the nullifier table's probe found no slot"
                             : err & 2 ? ": a nullifier slot holds a later entry than the one that stopped at it"
                                       : err & 4 ? ": the account table's probe found no slot"
                                                 : err & 8 ? ": a table slot holds no log entry"
                                                           : ": a transfer number in the log is not a field element") +
                    " (an internal invariant broke)");
}

int upload_roots(qp_ledger *l) {
  hipStream_t s = l->ctx->stream;
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  QP_HIP_TRY(l, hipMemcpyAsync(l->d_roots.p, l->screen.roots.data(), l->screen.roots.size() * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  return QP_OK;
}

int batch_buffers(qp_ledger *l, uint32_t n) {
  if (n <= l->batch_room) return QP_OK;
  l->batch_room = 0;
  QP_HIP_TRY(l, l->d_pis.alloc((size_t)n * ql::NPI));
  QP_HIP_TRY(l, l->d_ver.alloc(((size_t)n + 1) / 2));
  QP_HIP_TRY(l, l->d_res.alloc((size_t)n * 3));
  QP_HIP_TRY(l, l->d_blk.alloc(((size_t)qpk::ledger_blocks(n) + 2) / 2));
  QP_HIP_TRY(l, l->d_pos.alloc(((size_t)n + 1) / 2));
  QP_HIP_TRY(l, l->d_stay.alloc(((size_t)n + 1) / 2));
  l->batch_room = n;
  return QP_OK;
}

// The device steps of one batch.  The raw inputs go up; screen and scan run; the host reads the
// admitted count k back and refuses an overflow (*refused, nothing of the ledger written yet);
// then pack, insert, resolve and credit.
int cast_device(qp_ledger *l, const char *fn, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                ql::Result *out, bool *refused) {
  qp_ctx *c = l->ctx;
  hipStream_t s = c->stream;
  QP_HIP_TRY(l, hipSetDevice(c->device));
  for (hipEvent_t &e : l->ev.e)
    if (!e) QP_HIP_TRY(l, hipEventCreate(&e));
  if (int rc = batch_buffers(l, n)) return rc;
  const qpk::LedgerDev d = l->t.dev();
  qpk::LedgerCounters *ctr = l->d_ctr.as<qpk::LedgerCounters>();
  qpk::LedgerCounters now;
  qpk::LedgerScreen sc;
  sc.roots = l->d_roots.p;
  sc.nroots = l->screen.nroots();
  sc.has_padding = l->screen.has_padding;
  memcpy(sc.padding, l->screen.padding, sizeof sc.padding);
  const uint32_t nb = qpk::ledger_blocks(n);
  uint32_t *blk = l->d_blk.as<uint32_t>(), *d_ver = verdicts ? l->d_ver.as<uint32_t>() : nullptr;
  qpk::LedgerResult *res = l->d_res.as<qpk::LedgerResult>();
  uint32_t k = 0;
  QP_HIP_TRY(l, hipEventRecord(l->ev.e[0], s));
  QP_HIP_TRY(l, hipMemcpyAsync(l->d_pis.p, pis, (size_t)n * ql::NPI * 8, hipMemcpyHostToDevice, s));
  if (verdicts) QP_HIP_TRY(l, hipMemcpyAsync(d_ver, verdicts, (size_t)n * 4, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(l, hipEventRecord(l->ev.e[1], s));
  qpk::ledger_screen(sc, l->d_pis.p, d_ver, n, l->cast, res, blk, s);
  QP_HIP_TRY(l, hipGetLastError());
  qpk::ledger_scan(blk, nb, blk + nb, s);
  QP_HIP_TRY(l, hipGetLastError());
  QP_HIP_TRY(l, hipMemcpyAsync(&k, blk + nb, 4, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  if (k > n)
    return refuse(l, l->BROKEN, std::string(fn) + ": the pack's scan counted more admitted transfers than were cast (an "
                                                  "internal invariant broke)");
  if (k > l->capacity - l->count) {
    *refused = true;
    return over_capacity(l, fn, k);
  }
  qpk::ledger_pack(d, l->d_pis.p, res, blk, n, (uint32_t)l->count, l->d_pos.as<uint32_t>(), s);
  QP_HIP_TRY(l, hipGetLastError());
  qpk::ledger_insert(d, (uint32_t)l->count, k, l->d_stay.as<uint32_t>(), ctr, s);
  QP_HIP_TRY(l, hipGetLastError());
  qpk::ledger_resolve(d, (uint32_t)l->count, k, l->d_stay.as<uint32_t>(), l->d_pos.as<uint32_t>(), res, ctr, s);
  QP_HIP_TRY(l, hipGetLastError());
  QP_HIP_TRY(l, hipEventRecord(l->ev.e[2], s));
  QP_HIP_TRY(l, hipMemcpyAsync(out, res, (size_t)n * sizeof(ql::Result), hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipMemcpyAsync(&now, ctr, sizeof now, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  QP_HIP_TRY(l, hipEventElapsedTime(&l->ms[0], l->ev.e[0], l->ev.e[1]));
  QP_HIP_TRY(l, hipEventElapsedTime(&l->ms[1], l->ev.e[1], l->ev.e[2]));
  if (int rc = error_word(l, fn, now.err)) return rc;
  l->count += k;
  l->credited = now.credited;
  l->accounts = now.accounts;
  if (k) l->payee_valid = false;
  return QP_OK;
}

// pis [n][16], verdicts (may be null): screen, pack, refuse an overflow, settle
int cast_screened(qp_ledger *l, const char *fn, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                  ql::Result *out) {
  if (l->ctx) {
    bool refused = false;
    const int rc = cast_device(l, fn, pis, verdicts, n, out, &refused);
    if (rc) {
      if (!refused) l->dead = true;
      return rc;
    }
  } else {
    ql::screen_and_pack(l->screen, pis, verdicts, n, l->cast, out, l->pk);
    if (l->pk.size() > l->cap() - l->admitted()) return over_capacity(l, fn, l->pk.size());
    l->host.admit_packed(l->pk, out);
  }
  l->cast += n;
  return QP_OK;
}

int query_buffers(qp_ledger *l) {
  if (l->d_q.p) return QP_OK;
  QP_HIP_TRY(l, l->d_qsum.alloc((size_t)QUERY_BATCH * 4));
  QP_HIP_TRY(l, l->d_qaux.alloc(QUERY_BATCH));
  QP_HIP_TRY(l, l->d_q.alloc((size_t)QUERY_BATCH * 4));
  return QP_OK;
}

int find_device(qp_ledger *l, const uint64_t *nullifiers, uint32_t k, uint64_t *seq_out) {
  hipStream_t s = l->ctx->stream;
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  if (int rc = query_buffers(l)) return rc;
  qpk::LedgerCounters *ctr = l->d_ctr.as<qpk::LedgerCounters>();
  std::vector<uint32_t> h(std::min(k, QUERY_BATCH));
  uint32_t err = 0;
  for (uint32_t done = 0; done < k;) {
    const uint32_t nb = std::min(QUERY_BATCH, k - done);
    QP_HIP_TRY(l, hipMemcpyAsync(l->d_q.p, nullifiers + (size_t)done * 4, (size_t)nb * 32, hipMemcpyHostToDevice, s));
    qpk::ledger_find(l->t.dev(), (uint32_t)l->count, l->d_q.p, nb, l->d_qaux.as<uint32_t>(), ctr, s);
    QP_HIP_TRY(l, hipGetLastError());
    QP_HIP_TRY(l, hipMemcpyAsync(h.data(), l->d_qaux.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipMemcpyAsync(&err, &ctr->err, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipStreamSynchronize(s));
    if (int rc = error_word(l, "qp_ledger_find", err)) return rc;
    for (uint32_t i = 0; i < nb; i++) seq_out[done + i] = h[i] == ql::EMPTY ? ql::NOT_FOUND : h[i];
    done += nb;
  }
  return QP_OK;
}

int totals_device(qp_ledger *l, const uint64_t *accounts, uint32_t k, uint64_t *sums, uint8_t *found) {
  hipStream_t s = l->ctx->stream;
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  if (int rc = query_buffers(l)) return rc;
  qpk::LedgerCounters *ctr = l->d_ctr.as<qpk::LedgerCounters>();
  std::vector<uint32_t> h(std::min(k, QUERY_BATCH));
  uint32_t err = 0;
  for (uint32_t done = 0; done < k;) {
    const uint32_t nb = std::min(QUERY_BATCH, k - done);
    QP_HIP_TRY(l, hipMemcpyAsync(l->d_q.p, accounts + (size_t)done * 4, (size_t)nb * 32, hipMemcpyHostToDevice, s));
    qpk::ledger_totals(l->t.dev(), (uint32_t)l->count, l->d_q.p, nb, l->d_qsum.as<unsigned long long>(),
                       l->d_qaux.as<uint32_t>(), ctr, s);
    QP_HIP_TRY(l, hipGetLastError());
    if (sums) QP_HIP_TRY(l, hipMemcpyAsync(sums + (size_t)done * 4, l->d_qsum.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipMemcpyAsync(h.data(), l->d_qaux.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipMemcpyAsync(&err, &ctr->err, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipStreamSynchronize(s));
    if (int rc = error_word(l, "qp_ledger_totals_for", err)) return rc;
    if (found)
      for (uint32_t i = 0; i < nb; i++) found[done + i] = h[i] != 0;
    done += nb;
  }
  return QP_OK;
}

// d_payee = the log entries that own their account slot, in log order: the accounts in the order of
// their first credited entry
int payees_device(qp_ledger *l) {
  if (l->payee_valid) return QP_OK;
  hipStream_t s = l->ctx->stream;
  const uint32_t count = (uint32_t)l->count, nb = qpk::ledger_blocks(count);
  if (l->payee_room < l->count) {
    l->payee_room = 0;
    QP_HIP_TRY(l, l->d_pblk.alloc(((size_t)nb + 2) / 2));
    QP_HIP_TRY(l, l->d_payee.alloc((l->count + 1) / 2));
    l->payee_room = l->count;
  }
  if (count) {
    uint32_t *blk = l->d_pblk.as<uint32_t>(), total = 0;
    qpk::ledger_payee_count(l->t.dev(), count, blk, s);
    QP_HIP_TRY(l, hipGetLastError());
    qpk::ledger_scan(blk, nb, blk + nb, s);
    QP_HIP_TRY(l, hipGetLastError());
    qpk::ledger_payee_write(l->t.dev(), count, blk, l->d_payee.as<uint32_t>(), s);
    QP_HIP_TRY(l, hipGetLastError());
    QP_HIP_TRY(l, hipMemcpyAsync(&total, blk + nb, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipStreamSynchronize(s));
    if (total != l->accounts)
      return refuse(l, l->BROKEN, "qp_ledger_payouts: " + std::to_string(total) + " entries own an account slot, the ledger counts " +
                                      std::to_string(l->accounts) + " accounts (an internal invariant broke)");
  }
  l->payee_valid = true;
  return QP_OK;
}

int payouts_device(qp_ledger *l, uint64_t first, uint64_t k, uint64_t *accounts, uint64_t *sums, uint64_t *first_seq) {
  hipStream_t s = l->ctx->stream;
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  if (int rc = query_buffers(l)) return rc;
  if (int rc = payees_device(l)) return rc;
  for (uint64_t done = 0; done < k;) {
    const uint32_t nb = (uint32_t)std::min<uint64_t>(QUERY_BATCH, k - done);
    qpk::ledger_payouts(l->t.dev(), l->d_payee.as<uint32_t>() + first + done, nb, l->d_q.p,
                        l->d_qsum.as<unsigned long long>(), l->d_qaux.p, s);
    QP_HIP_TRY(l, hipGetLastError());
    if (accounts) QP_HIP_TRY(l, hipMemcpyAsync(accounts + done * 4, l->d_q.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    if (sums) QP_HIP_TRY(l, hipMemcpyAsync(sums + done * 4, l->d_qsum.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    if (first_seq) QP_HIP_TRY(l, hipMemcpyAsync(first_seq + done, l->d_qaux.p, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipStreamSynchronize(s));
    done += nb;
  }
  return QP_OK;
}

int reserve_device(qp_ledger *l, uint64_t new_capacity) {
  // a new log and new tables beside the old; the ledger moves over only once all of it succeeded
  qp_ctx *c = l->ctx;
  hipStream_t s = c->stream;
  LedgerTables nt;
  qpk::LedgerCounters now;
  QP_HIP_TRY(l, hipSetDevice(c->device));
  if (int rc = qla::alloc_tables({l->err}, s, new_capacity, nt)) return rc;
  const qpk::LedgerDev od = l->t.dev(), nd = nt.dev();
  qpk::LedgerCounters *ctr = l->d_ctr.as<qpk::LedgerCounters>();
  if (l->count) {
    QP_HIP_TRY(l, hipMemcpyAsync(nd.nullifier, od.nullifier, l->count * 32, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(l, hipMemcpyAsync(nd.number, od.number, l->count * 8, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(l, hipMemcpyAsync(nd.amount, od.amount, l->count * 16, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(l, hipMemcpyAsync(nd.account, od.account, l->count * 32, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(l, hipMemcpyAsync(nd.flags, od.flags, l->count, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(l, hipMemcpyAsync(nd.astay, od.astay, l->count * 4, hipMemcpyDeviceToDevice, s));
    qpk::ledger_rebuild(nd, (uint32_t)l->count, ctr, s);
    QP_HIP_TRY(l, hipGetLastError());
  }
  QP_HIP_TRY(l, hipMemcpyAsync(&now, ctr, sizeof now, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  if (int rc = error_word(l, "qp_ledger_reserve", now.err)) return device_step(l, rc);
  l->t = std::move(nt);
  l->capacity = new_capacity;
  l->payee_valid = false;  // the payees are the same entries, but the list is cheap and this keeps one rule
  l->lc.drop();
  return QP_OK;
}

// the log commitment up to the admitted count (> 0; the caller checks), on either path
int commit(qp_ledger *l) {
  const char *fn = "qp_ledger_commit_log";
  if (!l->ctx) return l->lc.commit(l->host) ? QP_OK : error_word(l, fn, qpk::LEDGER_ERR_NUMBER);
  qpk::LedgerCounters *ctr = l->d_ctr.as<qpk::LedgerCounters>();
  auto leaves = [&](uint32_t first, uint32_t end, uint64_t *dig) {
    qpk::ledger_leaves(l->t.dev(), first, end, dig, ctr, l->ctx->stream);
  };
  uint32_t word = 0;
  if (int rc = l->lc.commit(l->ctx, l->err, fn, l->BROKEN, l->count, l->capacity, leaves, &ctr->err, &word)) return rc;
  return error_word(l, fn, word);
}

// the set commitment over the credited entries of the log as it stands, on either path.  A ledger's
// log never credits one nullifier twice: a duplicate member is the defensive error.
int commit_members(qp_ledger *l, const char *fn) {
  uint64_t dup = ql::NOT_FOUND;
  if (!l->ctx) {
    l->sc.commit_host(l->host.nullifier.data(), l->host.flags.data(), l->host.count(), ql::FLAG_CREDITED, &dup);
  } else {
    const qpk::LedgerDev d = l->t.dev();
    if (int rc = l->sc.commit_device(l->ctx, l->err, d.nullifier, d.flags, l->count, ql::FLAG_CREDITED, &dup)) {
      l->err = std::string(fn) + ": " + l->err;
      return rc;
    }
  }
  if (dup == ql::NOT_FOUND) return QP_OK;
  l->dead = true;
  return refuse(l, l->BROKEN, std::string(fn) + ": entry " + std::to_string(dup) +
                                  " is credited and an earlier credited entry has its nullifier (an internal invariant broke)");
}

// The device half of a restore, over the fresh ledger's own log and tables (sized for its capacity):
// the audit's passes up to its resolve (ledger_audit_device.h), then this call's own synchronise.  What
// those launches leave is a live ledger's state (both tables, astay, the sums), so no kernel of the
// restore's own is needed; the counts go from the audit's report into the ledger's counters.  The
// root, when one is expected, is the restored ledger's own commit afterwards.
int restore_device(qp_ledger *l, const ql::AuditLog &g, ql::AuditFacts &f, bool *canonical) {
  qp_ctx *c = l->ctx;
  hipStream_t s = c->stream;
  const uint64_t n = g.n;
  qla::AuditPasses a;
  const qpk::LedgerAuditDev &h = a.h;
  bool screened = false;
  *canonical = false;
  QP_HIP_TRY(l, hipSetDevice(c->device));
  if (int rc = qla::audit_screen_insert_resolve({l->err}, s, g, l->t.dev(), a, &screened)) return rc;
  if (!screened) {
    f.non_canonical = h.non_canonical;
    return QP_OK;
  }
  QP_HIP_TRY(l, hipMemcpyAsync(&a.h, a.rep(), sizeof h, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  if (int rc = error_word(l, "qp_ledger_restore", h.ctr.err)) return rc;
  if (h.ctr.credited > n || h.ctr.accounts > h.ctr.credited)
    return refuse(l, l->BROKEN, "qp_ledger_restore: the resolve counted more credited entries or accounts than the log has (an "
                                "internal invariant broke)");
  a.rule_facts(f);
  f.credited = h.ctr.credited;
  f.accounts = h.ctr.accounts;
  const qpk::LedgerCounters now{h.ctr.credited, h.ctr.accounts, 0, 0};
  QP_HIP_TRY(l, hipMemcpyAsync(l->d_ctr.p, &now, sizeof now, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  l->count = n;
  l->credited = now.credited;
  l->accounts = now.accounts;
  *canonical = true;
  return QP_OK;
}

int entries_at_device(qp_ledger *l, const uint64_t *seqs, uint32_t k, uint64_t *nullifiers, uint64_t *numbers,
                      uint32_t *amounts, uint64_t *accounts, uint8_t *flags) {
  hipStream_t s = l->ctx->stream;
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  if (int rc = query_buffers(l)) return rc;
  if (!l->d_gnum.p) {
    QP_HIP_TRY(l, l->d_gacc.alloc((size_t)QUERY_BATCH * 4));
    QP_HIP_TRY(l, l->d_gamt.alloc((size_t)QUERY_BATCH * 2));
    QP_HIP_TRY(l, l->d_gflag.alloc(QUERY_BATCH / 8));
    QP_HIP_TRY(l, l->d_gnum.alloc(QUERY_BATCH));
  }
  for (uint32_t done = 0; done < k;) {
    const uint32_t nb = std::min(QUERY_BATCH, k - done);
    QP_HIP_TRY(l, hipMemcpyAsync(l->d_q.p, seqs + done, (size_t)nb * 8, hipMemcpyHostToDevice, s));
    qpk::ledger_gather(l->t.dev(), l->d_q.p, nb, l->d_qsum.p, l->d_gnum.p, l->d_gamt.as<uint32_t>(), l->d_gacc.p,
                       l->d_gflag.as<uint8_t>(), s);
    QP_HIP_TRY(l, hipGetLastError());
    if (nullifiers)
      QP_HIP_TRY(l, hipMemcpyAsync(nullifiers + (size_t)done * 4, l->d_qsum.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    if (numbers) QP_HIP_TRY(l, hipMemcpyAsync(numbers + done, l->d_gnum.p, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    if (amounts)
      QP_HIP_TRY(l, hipMemcpyAsync(amounts + (size_t)done * 4, l->d_gamt.p, (size_t)nb * 16, hipMemcpyDeviceToHost, s));
    if (accounts)
      QP_HIP_TRY(l, hipMemcpyAsync(accounts + (size_t)done * 4, l->d_gacc.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    if (flags) QP_HIP_TRY(l, hipMemcpyAsync(flags + done, l->d_gflag.p, nb, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(l, hipStreamSynchronize(s));
    done += nb;
  }
  return QP_OK;
}

// what both claims calls refuse first: a dead handle, a range outside the log (payouts_between's words)
int claims_front(qp_ledger *l, const char *fn, uint64_t m0, uint64_t m1) {
  if (l->dead) return dead_handle(l, fn);
  uint64_t count = 0;
  const std::string why = ql::round_refusal(l->admitted(), m0, m1, 0, nullptr, nullptr, nullptr, &count);
  return why.empty() ? QP_OK : refuse(l, QP_ERR_ARG, std::string(fn) + ": " + why);
}

// the claims commitment of log range [m0, m1) (inside the log; the caller checked), on either path
int commit_claims(qp_ledger *l, const char *fn, uint64_t m0, uint64_t m1) {
  if (!l->ctx) {
    const ql::HostLedger &h = l->host;
    l->cc.commit_host(h.account.data(), h.amount.data(), h.flags.data(), m0, m1);
    return QP_OK;
  }
  const qpk::LedgerDev d = l->t.dev();
  const int rc = l->cc.commit_device(l->ctx, l->err, d.account + m0 * 4, d.amount + m0 * 4, d.flags + m0, m0, m1);
  if (rc) l->err = std::string(fn) + ": " + l->err;
  return rc == QP_ERR_OOM ? rc : device_step(l, rc);  // the buffers are the commitment's own: the ledger stands
}

}  // namespace

extern "C" {

int qp_ledger_new(qp_ctx *c, const uint64_t *roots, uint32_t nroots, const uint64_t *padding_pis, uint64_t capacity,
                  qp_ledger **out) {
  if (!out) return QP_ERR_ARG;
  *out = nullptr;
  if (!roots) return refuse_new(c, "null roots");
  if (!nroots || nroots > ql::MAX_ROOTS)
    return refuse_new(c, std::to_string(nroots) + " accepted roots: a ledger needs 1 to " + std::to_string(ql::MAX_ROOTS));
  if (!ql::canonical(roots, (size_t)nroots * 4)) return refuse_new(c, "a root is not four canonical field elements");
  if (padding_pis && !ql::canonical(padding_pis, ql::NPI))
    return refuse_new(c, "the padding inputs are not 16 canonical field elements");
  if (!capacity || capacity > ql::MAX_CAPACITY)
    return refuse_new(c, "capacity " + std::to_string(capacity) + ": it must be 1 to 2^31 admitted transfers");
  std::unique_ptr<qp_ledger> l(new (std::nothrow) qp_ledger);
  if (!l) return QP_ERR_OOM;
  l->ctx = c;
  if (padding_pis) {
    l->screen.has_padding = true;
    memcpy(l->screen.padding, padding_pis, sizeof l->screen.padding);
  }
  try {
    for (uint32_t i = 0; i < nroots; i++)
      if (!l->screen.accepts(roots + 4 * i)) l->screen.add_root(roots + 4 * i);
    if (!c) {
      l->host.open(capacity);
      *out = l.release();
      return QP_OK;
    }
  } catch (const std::bad_alloc &) {
    g_new_err.text = "qp_ledger_new: out of host memory";
    return QP_ERR_OOM;
  }
  int rc = QP_OK;
  auto device_open = [&]() -> int {
    QP_HIP_TRY(l, hipSetDevice(c->device));
    if ((rc = qla::alloc_tables({l->err}, c->stream, capacity, l->t))) return rc;
    QP_HIP_TRY(l, l->d_roots.alloc((size_t)ql::MAX_ROOTS * 4));
    QP_HIP_TRY(l, l->d_ctr.alloc((sizeof(qpk::LedgerCounters) + 7) / 8));
    QP_HIP_TRY(l, l->d_audit.alloc(6));
    QP_HIP_TRY(l, hipMemsetAsync(l->d_ctr.p, 0, sizeof(qpk::LedgerCounters), c->stream));
    return upload_roots(l.get());
  };
  if ((rc = device_open())) {
    g_new_err.set(c, "qp_ledger_new: " + l->err);
    return rc;
  }
  l->capacity = capacity;
  *out = l.release();
  return QP_OK;
}

void qp_ledger_free(qp_ledger *l) {
  if (!l) return;
  if (l->ctx) (void)hipSetDevice(l->ctx->device);
  delete l;
}

const char *qp_ledger_last_error(const qp_ledger *l) { return l ? l->err.c_str() : g_new_err.text.c_str(); }

int qp_ledger_accept_root(qp_ledger *l, const uint64_t root[4]) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_accept_root");
  if (!root || !ql::canonical(root, 4)) {
    l->err = "qp_ledger_accept_root: the root must be four canonical field elements";
    return QP_ERR_ARG;
  }
  if (l->screen.accepts(root)) return QP_OK;
  if (l->screen.nroots() >= ql::MAX_ROOTS) {
    l->err = "qp_ledger_accept_root: the ledger already accepts " + std::to_string(ql::MAX_ROOTS) + " roots, the most";
    return QP_ERR_ARG;
  }
  try {
    l->screen.add_root(root);
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_accept_root");
  }
  return l->ctx ? device_step(l, upload_roots(l)) : QP_OK;
}

int qp_ledger_cast_public(qp_ledger *l, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                          qp_transfer_result *out) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_cast_public");
  if (!n) return QP_OK;
  if (n > ql::MAX_BATCH) {
    l->err = "qp_ledger_cast_public: " + std::to_string(n) + " transfers in one call; the most is 2^22";
    return QP_ERR_ARG;
  }
  if (!pis || !out) return null_buffer(l, "qp_ledger_cast_public");
  try {
    return cast_screened(l, "qp_ledger_cast_public", pis, verdicts, n, reinterpret_cast<ql::Result *>(out));
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_cast_public");
  }
}

int qp_ledger_cast(qp_ledger *l, struct qp_verifier *v, const uint8_t *const *proofs, const size_t *lens, uint32_t n,
                   qp_transfer_result *out) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_cast");
  if (int rc = check_verifier(l, "qp_ledger_cast", v, ql::NPI, "the Wormhole circuit's")) return rc;
  if (!n) return QP_OK;
  if (n > ql::MAX_BATCH) {
    l->err = "qp_ledger_cast: " + std::to_string(n) + " transfers in one call; the most is 2^22";
    return QP_ERR_ARG;
  }
  if (!proofs || !lens || !out) return null_buffer(l, "qp_ledger_cast");
  try {
    std::vector<uint32_t> verdicts;
    std::vector<uint64_t> pis;
    if (int rc = verify_and_gather(l, "qp_ledger_cast", v, proofs, lens, n, ql::NPI, verdicts, pis)) return rc;
    return cast_screened(l, "qp_ledger_cast", pis.data(), verdicts.data(), n, reinterpret_cast<ql::Result *>(out));
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_cast");
  }
}

int qp_ledger_reserve(qp_ledger *l, uint64_t new_capacity) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_reserve");
  if (int rc = check_reserve(l, "qp_ledger_reserve", new_capacity)) return rc;
  if (new_capacity == l->cap()) return QP_OK;
  if (l->ctx) return reserve_device(l, new_capacity);
  try {
    l->host.reserve(new_capacity);
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_reserve");
  }
  l->lc.drop();
  return QP_OK;
}

int qp_ledger_state(const qp_ledger *l, uint64_t *cast, uint64_t *admitted, uint64_t *credited, uint64_t *accounts,
                    uint64_t *capacity) {
  if (!l) return QP_ERR_ARG;
  if (cast) *cast = l->cast;
  if (admitted) *admitted = l->admitted();
  if (credited) *credited = l->ncredited();
  if (accounts) *accounts = l->naccounts();
  if (capacity) *capacity = l->cap();
  return QP_OK;
}

int qp_ledger_find(qp_ledger *l, const uint64_t *nullifiers, uint32_t k, uint64_t *seq_out) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_find");
  if (!k) return QP_OK;
  if (!nullifiers || !seq_out) return null_buffer(l, "qp_ledger_find");
  if (int rc = canonical_keys(l, "qp_ledger_find", "nullifier", nullifiers, k)) return rc;
  if (!l->ctx) {
    for (uint32_t i = 0; i < k; i++) seq_out[i] = l->host.find(nullifiers + (size_t)i * 4);
    return QP_OK;
  }
  try {
    return device_step(l, find_device(l, nullifiers, k, seq_out));
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_find");
  }
}

int qp_ledger_entries(qp_ledger *l, uint64_t first, uint64_t k, uint64_t *nullifiers, uint64_t *numbers,
                      uint32_t *amounts, uint64_t *accounts, uint8_t *flags) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_entries");
  if (int rc = check_range(l, "qp_ledger_entries", first, k)) return rc;
  if (!k) return QP_OK;
  if (!l->ctx) {
    const ql::HostLedger &h = l->host;
    if (nullifiers) memcpy(nullifiers, &h.nullifier[first * 4], k * 32);
    if (numbers) memcpy(numbers, &h.number[first], k * 8);
    if (amounts) memcpy(amounts, &h.amount[first * 4], k * 16);
    if (accounts) memcpy(accounts, &h.account[first * 4], k * 32);
    if (flags) memcpy(flags, &h.flags[first], k);
    return QP_OK;
  }
  hipStream_t s = l->ctx->stream;
  const qpk::LedgerDev d = l->t.dev();
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  if (nullifiers) QP_HIP_TRY(l, hipMemcpyAsync(nullifiers, d.nullifier + first * 4, k * 32, hipMemcpyDeviceToHost, s));
  if (numbers) QP_HIP_TRY(l, hipMemcpyAsync(numbers, d.number + first, k * 8, hipMemcpyDeviceToHost, s));
  if (amounts) QP_HIP_TRY(l, hipMemcpyAsync(amounts, d.amount + first * 4, k * 16, hipMemcpyDeviceToHost, s));
  if (accounts) QP_HIP_TRY(l, hipMemcpyAsync(accounts, d.account + first * 4, k * 32, hipMemcpyDeviceToHost, s));
  if (flags) QP_HIP_TRY(l, hipMemcpyAsync(flags, d.flags + first, k, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_ledger_payouts(qp_ledger *l, uint64_t first, uint64_t k, uint64_t *accounts, uint64_t *sums,
                      uint64_t *first_seq) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_payouts");
  if (first > l->naccounts() || k > l->naccounts() - first) {
    l->err = "qp_ledger_payouts: accounts [" + std::to_string(first) + ", " + std::to_string(first) + " + " +
             std::to_string(k) + ") are outside the " + std::to_string(l->naccounts()) + " credited so far";
    return QP_ERR_ARG;
  }
  if (!k) return QP_OK;
  if (l->ctx) return device_step(l, payouts_device(l, first, k, accounts, sums, first_seq));
  const ql::HostLedger &h = l->host;
  for (uint64_t i = 0; i < k; i++) {
    const uint32_t seq = h.payee[first + i];
    if (accounts) memcpy(accounts + i * 4, &h.account[(size_t)seq * 4], 32);
    if (sums) memcpy(sums + i * 4, &h.sum[(size_t)h.astay[seq] * 4], 32);
    if (first_seq) first_seq[i] = seq;
  }
  return QP_OK;
}

int qp_ledger_payouts_between(qp_ledger *l, uint64_t m0, uint64_t m1, uint64_t cap, uint64_t *accounts, uint64_t *sums,
                              uint64_t *first_seq, uint64_t *count) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_payouts_between");
  const std::string why = ql::round_refusal(l->admitted(), m0, m1, cap, accounts, sums, first_seq, count);
  if (!why.empty()) {
    l->err = "qp_ledger_payouts_between: " + why;
    return QP_ERR_ARG;
  }
  if (m0 == m1) {
    *count = 0;
    return QP_OK;
  }
  try {
    if (l->ctx) {
      const qpk::LedgerDev d = l->t.dev();
      const int rc = qla::rounds_device(l->ctx, l->err, d.account + m0 * 4, d.amount + m0 * 4, d.flags + m0, m1 - m0, m0,
                                        cap, accounts, sums, first_seq, count);
      if (rc) l->err = "qp_ledger_payouts_between: " + l->err;
      return rc == QP_ERR_OOM ? rc : device_step(l, rc);  // the scratch is the call's own: the ledger stands
    }
    const ql::HostLedger &h = l->host;
    ql::RoundRows rows;
    ql::round_payouts_host(h.account.data(), h.amount.data(), h.flags.data(), m0, m1, rows);
    ql::round_store(rows, cap, accounts, sums, first_seq, count);
    return QP_OK;
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_payouts_between");
  }
}

int qp_ledger_totals_for(qp_ledger *l, const uint64_t *accounts, uint32_t k, uint64_t *sums, uint8_t *found) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_totals_for");
  if (!k) return QP_OK;
  if (!accounts) return null_buffer(l, "qp_ledger_totals_for");
  if (int rc = canonical_keys(l, "qp_ledger_totals_for", "account", accounts, k)) return rc;
  if (!l->ctx) {
    for (uint32_t i = 0; i < k; i++) {
      uint64_t s[4];
      const bool f = l->host.total_for(accounts + (size_t)i * 4, s);
      if (sums) memcpy(sums + (size_t)i * 4, s, 32);
      if (found) found[i] = f;
    }
    return QP_OK;
  }
  try {
    return device_step(l, totals_device(l, accounts, k, sums, found));
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, "qp_ledger_totals_for");
  }
}

int qp_ledger_recount(qp_ledger *l, uint64_t out[6]) {
  if (!l || !out) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_recount");
  if (!l->ctx) {
    l->host.recount(out);
    return QP_OK;
  }
  hipStream_t s = l->ctx->stream;
  QP_HIP_TRY(l, hipSetDevice(l->ctx->device));
  QP_HIP_TRY(l, hipMemsetAsync(l->d_audit.p, 0, 48, s));
  qpk::ledger_recount(l->t.dev(), (uint32_t)l->count, l->d_audit.as<unsigned long long>(), s);
  QP_HIP_TRY(l, hipGetLastError());
  QP_HIP_TRY(l, hipMemcpyAsync(out, l->d_audit.p, 48, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(l, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_ledger_commit_log(qp_ledger *l, uint64_t root_out[4], uint64_t *n_out) {
  return qph::commit_log(l, "qp_ledger_commit_log", commit, root_out, n_out);
}

int qp_ledger_entries_at(qp_ledger *l, const uint64_t *seqs, uint32_t k, uint64_t *nullifiers, uint64_t *numbers,
                         uint32_t *amounts, uint64_t *accounts, uint8_t *flags) {
  if (!l) return QP_ERR_ARG;
  if (l->dead) return dead_handle(l, "qp_ledger_entries_at");
  if (!k) return QP_OK;
  if (!seqs) return null_buffer(l, "qp_ledger_entries_at");
  if (int rc = check_seqs(l, "qp_ledger_entries_at", seqs, k)) return rc;
  if (l->ctx) return device_step(l, entries_at_device(l, seqs, k, nullifiers, numbers, amounts, accounts, flags));
  const ql::HostLedger &h = l->host;
  for (uint32_t i = 0; i < k; i++) {
    const size_t at = (size_t)seqs[i];
    if (nullifiers) memcpy(nullifiers + (size_t)i * 4, &h.nullifier[at * 4], 32);
    if (numbers) numbers[i] = h.number[at];
    if (amounts) memcpy(amounts + (size_t)i * 4, &h.amount[at * 4], 16);
    if (accounts) memcpy(accounts + (size_t)i * 4, &h.account[at * 4], 32);
    if (flags) flags[i] = h.flags[at];
  }
  return QP_OK;
}

int qp_ledger_receipts(qp_ledger *l, const uint64_t *seqs, uint32_t k, uint64_t *siblings, uint32_t *path_bits,
                       uint32_t *depth, uint64_t *leaves, uint64_t root_out[4], uint64_t *n_out) {
  return qph::receipts(l, "qp_ledger_receipts", commit, seqs, k, siblings, path_bits, depth, leaves, root_out, n_out);
}

int qp_ledger_roots_at(qp_ledger *l, const uint64_t *ms, uint32_t k, uint64_t *roots_out) {
  return qph::roots_at(l, "qp_ledger_roots_at", commit, ql::log_node, ms, k, roots_out);
}

int qp_ledger_restore(qp_ctx *c, const uint64_t *roots, uint32_t nroots, const uint64_t *padding_pis, uint64_t capacity,
                      const uint64_t *nullifiers, const uint64_t *numbers, const uint32_t *amounts,
                      const uint64_t *accounts, const uint8_t *flags, uint64_t n, uint64_t cast_count,
                      const uint64_t *expect_root, qp_ledger **out) {
  if (!out) return QP_ERR_ARG;
  auto refuse = [c](int rc, const std::string &why) {
    qla::set_ledgerless_error(c, "qp_ledger_restore: " + why);
    return rc;
  };
  if (n && (!nullifiers || !numbers || !amounts || !accounts || !flags)) return refuse(QP_ERR_ARG, "null log buffer");
  if (expect_root && (!n || !ql::canonical(expect_root, 4)))
    return refuse(QP_ERR_ARG, n ? "the expected root is not four canonical field elements" : "an empty log has no root");
  try {
    const std::string why = ql::restore_refusal(numbers, n, capacity, cast_count);
    if (!why.empty()) return refuse(QP_ERR_ARG, why);
    qp_ledger *fresh = nullptr;
    int rc = qp_ledger_new(c, roots, nroots, padding_pis, capacity, &fresh);
    if (rc) return rc;  // qp_ledger_new left its reason
    std::unique_ptr<qp_ledger, void (*)(qp_ledger *)> l(fresh, qp_ledger_free);
    l->cast = cast_count;
    if (!n) {
      *out = l.release();
      return QP_OK;
    }
    ql::AuditLog g;
    g.nullifiers = nullifiers, g.numbers = numbers, g.amounts = amounts, g.accounts = accounts, g.flags = flags, g.n = n;
    ql::AuditFacts f;
    ql::AuditReport r;
    bool canonical = false;
    if (c) {
      if ((rc = restore_device(l.get(), g, f, &canonical))) return refuse(rc, l->err);
    } else {
      ql::HostLog unused;  // the tree comes from the restored ledger's own commit below
      canonical = ql::audit_facts_host(g, ql::AuditClaims(), l->host, unused, f, capacity, false);
    }
    if (!canonical) {
      ql::audit_non_canonical(f.non_canonical, r);
    } else {
      ql::restore_verdict(f, n, nullptr, r);
      if (r.status == ql::AUDIT_OK && expect_root) {
        // The leaves and the tree, laid out for the capacity: the restored ledger's own first commit.
        // The tree is kept, so a commit_log() that follows returns this pair with nothing launched.
        if ((rc = commit(l.get()))) return refuse(rc, l->err);
        memcpy(f.root, l->lc.root, 32);
        ql::restore_verdict(f, n, expect_root, r);
      }
    }
    if (r.status != ql::AUDIT_OK) return refuse(QP_ERR_FORMAT, ql::audit_failure_text(r));
    *out = l.release();
    return QP_OK;
  } catch (const std::bad_alloc &) {
    return refuse(QP_ERR_OOM, "out of host memory");
  }
}

int qp_ledger_receipt_check(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t nullifier[4],
                            uint64_t number, const uint32_t amount[4], const uint64_t account[4], uint8_t flags,
                            const uint64_t *siblings, uint32_t path_bits, uint32_t depth) {
  if (!root || !nullifier || !amount || !account || !siblings) return QP_RECEIPT_NULL;
  return ql::receipt_check(root, n, seq, nullifier, number, amount, account, flags, siblings, path_bits, depth);
}

int qp_ledger_commit_set(qp_ledger *l, uint64_t root_out[4], uint64_t *m_out) {
  return qph::commit_set(l, "qp_ledger_commit_set", commit_members, root_out, m_out);
}

int qp_ledger_set_proofs(qp_ledger *l, const uint64_t *keys, uint32_t k, uint8_t *found, uint64_t *pos, uint64_t *lo_key,
                         uint64_t *lo_seq, uint64_t *lo_siblings, uint32_t *lo_bits, uint32_t *lo_depth,
                         uint64_t *hi_key, uint64_t *hi_seq, uint64_t *hi_siblings, uint32_t *hi_bits,
                         uint32_t *hi_depth, uint64_t root_out[4], uint64_t *m_out) {
  const SetCommit::Out o{found, pos, {lo_key, hi_key}, {lo_seq, hi_seq}, {lo_siblings, hi_siblings}, {lo_bits, hi_bits},
                         {lo_depth, hi_depth}};
  return qph::set_proofs(l, "qp_ledger_set_proofs", commit_members, keys, k, o, root_out, m_out);
}

int qp_ledger_commit_claims(qp_ledger *l, uint64_t m0, uint64_t m1, uint64_t root_out[4], uint64_t *count_out,
                            uint32_t total_out[5]) {
  const char *fn = "qp_ledger_commit_claims";
  if (!l) return QP_ERR_ARG;
  if (int rc = claims_front(l, fn, m0, m1)) return rc;
  try {
    if (int rc = commit_claims(l, fn, m0, m1)) return rc;
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, fn);
  }
  l->cc.triple(root_out, count_out, total_out);
  return QP_OK;
}

int qp_ledger_claims(qp_ledger *l, uint64_t m0, uint64_t m1, const uint64_t *accounts, uint32_t k, uint8_t *found,
                     uint64_t *pos, uint64_t *lo_account, uint32_t *lo_total, uint64_t *lo_first_seq,
                     uint64_t *lo_siblings, uint32_t *lo_bits, uint32_t *lo_depth, uint64_t *hi_account,
                     uint32_t *hi_total, uint64_t *hi_first_seq, uint64_t *hi_siblings, uint32_t *hi_bits,
                     uint32_t *hi_depth, uint64_t root_out[4], uint64_t *count_out) {
  const char *fn = "qp_ledger_claims";
  if (!l) return QP_ERR_ARG;
  if (int rc = claims_front(l, fn, m0, m1)) return rc;
  const ClaimsCommit::Out o{found,
                            pos,
                            {lo_account, hi_account},
                            {lo_total, hi_total},
                            {lo_first_seq, hi_first_seq},
                            {lo_siblings, hi_siblings},
                            {lo_bits, hi_bits},
                            {lo_depth, hi_depth}};
  bool null = !accounts || !found || !pos;
  for (int sl = 0; sl < 2; sl++)
    null = null || !o.account[sl] || !o.total[sl] || !o.first_seq[sl] || !o.sib[sl] || !o.bits[sl] || !o.depth[sl];
  if (k && null) return null_buffer(l, fn);
  if (int rc = canonical_keys(l, fn, "account", accounts, k)) return rc;
  try {
    if (int rc = commit_claims(l, fn, m0, m1)) return rc;
    l->cc.triple(root_out, count_out, nullptr);
    if (!k) return QP_OK;
    return device_step(l, l->cc.proofs(l->ctx, l->err, accounts, k, o));
  } catch (const std::bad_alloc &) {
    return bad_alloc(l, fn);
  }
}

int qp_ledger_cast_times(const qp_ledger *l, double ms[2]) {
  if (!l || !ms) return QP_ERR_ARG;
  ms[0] = l->ms[0];
  ms[1] = l->ms[1];
  return QP_OK;
}

}  // extern "C"
