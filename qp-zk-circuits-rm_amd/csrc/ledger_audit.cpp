// ledger_audit.cpp — qp_ledger_log_audit (qpgpu.h), and the passes over an
// uploaded log that it shares with qp_ledger_restore (ledger.cpp):
// qla::audit_screen_insert_resolve.  An audit needs no ledger: with a context
// the log is uploaded into tables of this call's own (ledger_audit_device.h's
// LedgerTables), which take it whole (ledger.hip's insert, probes, recount and
// payee compaction, with the audit's three kernels in between), the tree is
// log_commit.h's whole-log form, and the verdict is ledger_audit.h's, the same
// the host path reaches.
#include "../../include/qpgpu.h"
#include <string.h>
#include <algorithm>
#include <new>
#include <string>
#include <vector>
#include "acc_tree.h"
#include "ledger_audit.h"
#include "ledger_audit_device.h"
#include "ledger_kernels.h"
#include "log_commit.h"

static_assert(sizeof(qp_ledger_audit_report) == sizeof(ql::AuditReport) && sizeof(ql::AuditReport) == 104,
              "qp_ledger_audit_report layout");
static_assert(QP_LEDGER_AUDIT_OK == ql::AUDIT_OK && QP_LEDGER_AUDIT_NON_CANONICAL == ql::AUDIT_NON_CANONICAL &&
                  QP_LEDGER_AUDIT_ORDER == ql::AUDIT_ORDER && QP_LEDGER_AUDIT_CREDIT_RULE == ql::AUDIT_CREDIT_RULE &&
                  QP_LEDGER_AUDIT_TOTALS == ql::AUDIT_TOTALS && QP_LEDGER_AUDIT_PAYOUTS == ql::AUDIT_PAYOUTS &&
                  QP_LEDGER_AUDIT_ROOT == ql::AUDIT_ROOT && QP_LEDGER_AUDIT_COMMITMENT == ql::AUDIT_COMMITMENT,
              "qp_ledger_audit_status and ledger_audit.h differ");

namespace qla {

int audit_screen_insert_resolve(AccErr e, hipStream_t s, const ql::AuditLog &g, const qpk::LedgerDev &d, AuditPasses &a,
                                bool *canonical) {
  const uint64_t n = g.n;
  *canonical = false;
  QP_HIP_TRY(&e, a.d_rep.alloc((sizeof(qpk::LedgerAuditDev) + 7) / 8));
  QP_HIP_TRY(&e, a.d_stay.alloc((size_t)((n + 1) / 2)));
  QP_HIP_TRY(&e, hipMemcpyAsync(d.nullifier, g.nullifiers, (size_t)n * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(&e, hipMemcpyAsync(d.number, g.numbers, (size_t)n * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(&e, hipMemcpyAsync(d.amount, g.amounts, (size_t)n * 16, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(&e, hipMemcpyAsync(d.account, g.accounts, (size_t)n * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(&e, hipMemcpyAsync(d.flags, g.flags, (size_t)n, hipMemcpyHostToDevice, s));
  qpk::LedgerAuditDev &h = a.h;
  memset(&h, 0, sizeof h);
  h.credit_rule = ~0ull;
  h.non_canonical = h.order = h.payout = qpk::LEDGER_AUDIT_NO_SEQ;
  QP_HIP_TRY(&e, hipMemcpyAsync(a.rep(), &h, sizeof h, hipMemcpyHostToDevice, s));
  qpk::ledger_audit_screen(d, (uint32_t)n, a.rep(), s);
  QP_HIP_TRY(&e, hipGetLastError());
  QP_HIP_TRY(&e, hipMemcpyAsync(&h, a.rep(), sizeof h, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(&e, hipStreamSynchronize(s));
  if (h.non_canonical != qpk::LEDGER_AUDIT_NO_SEQ) return QP_OK;
  qpk::ledger_insert(d, 0, (uint32_t)n, a.d_stay.as<uint32_t>(), &a.rep()->ctr, s);
  QP_HIP_TRY(&e, hipGetLastError());
  qpk::ledger_audit_resolve(d, (uint32_t)n, a.d_stay.as<uint32_t>(), a.rep(), s);
  QP_HIP_TRY(&e, hipGetLastError());
  *canonical = true;
  return QP_OK;
}

}  // namespace qla

namespace {

// The passes over log [0, n) on the device.  Launch order on the one stream: screen (then a
// synchronise: on a non-canonical log nothing is hashed), the whole-log insert, the credit rule and the
// account sums (those three are audit_screen_insert_resolve, shared with the restore), the recount, the
// payees' compaction, the leaves and the levels above them; one more synchronise; then, with payouts
// claimed, their compare, which therefore reads the sums launches after the one that added them.
int audit_device(qp_ctx *c, const ql::AuditLog &g, const ql::AuditClaims &claims, ql::AuditReport &r) {
  hipStream_t s = c->stream;
  AccErr e{c->err};
  const uint64_t n = g.n;
  const uint32_t nb = qpk::ledger_blocks(n);
  QP_HIP_TRY(c, hipSetDevice(c->device));
  qla::LedgerTables t;
  DevBuf d_tot, d_blk, d_payee;
  if (int rc = qla::alloc_tables(e, s, n, t)) return rc;
  QP_HIP_TRY(c, d_tot.alloc(6));
  QP_HIP_TRY(c, d_blk.alloc(((size_t)nb + 2) / 2));
  QP_HIP_TRY(c, d_payee.alloc((size_t)((n + 1) / 2)));
  QP_HIP_TRY(c, hipMemsetAsync(d_tot.p, 0, 48, s));
  const qpk::LedgerDev d = t.dev();
  qla::AuditPasses a;
  bool canonical = false;
  if (int rc = qla::audit_screen_insert_resolve(e, s, g, d, a, &canonical)) return rc;
  if (!canonical) {
    ql::audit_non_canonical(a.h.non_canonical, r);
    return QP_OK;
  }
  qpk::LedgerAuditDev *rep = a.rep();
  qpk::LedgerAuditDev &h = a.h;
  uint32_t *blk = d_blk.as<uint32_t>(), *payee = d_payee.as<uint32_t>(), npayee = 0;
  uint64_t tot[6];
  ql::AuditFacts f;
  qpk::ledger_recount(d, (uint32_t)n, d_tot.as<unsigned long long>(), s);
  QP_HIP_TRY(c, hipGetLastError());
  qpk::ledger_payee_count(d, (uint32_t)n, blk, s);
  QP_HIP_TRY(c, hipGetLastError());
  qpk::ledger_scan(blk, nb, blk + nb, s);
  QP_HIP_TRY(c, hipGetLastError());
  qpk::ledger_payee_write(d, (uint32_t)n, blk, payee, s);
  QP_HIP_TRY(c, hipGetLastError());
  AccTree tree;
  qpk::AccLevels lv;
  auto leaves = [&](uint32_t first, uint32_t end, uint64_t *dig) { qpk::ledger_leaves(d, first, end, dig, &rep->ctr, s); };
  if (int rc = log_tree_whole(e, s, tree, n, leaves, lv, f.root)) return rc;
  QP_HIP_TRY(c, hipMemcpyAsync(&npayee, blk + nb, 4, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipMemcpyAsync(tot, d_tot.p, 48, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipMemcpyAsync(&h, rep, sizeof h, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(c, hipStreamSynchronize(s));
  if (h.ctr.err || npayee != h.ctr.accounts || tot[0] != h.ctr.credited) {
    c->err = std::string(h.ctr.err & 1   ? "the nullifier table's probe found no slot"
                         : h.ctr.err & 2 ? "a nullifier slot does not hold its nullifier's first entry"
                         : h.ctr.err & 4 ? "the account table's probe found no slot"
                         : h.ctr.err     ? "a transfer number in the log is not a field element"
                                         : "the payees and the account table disagree on the counts") +
             " (an internal invariant broke)";
    return QP_ERR_HIP;
  }
  tree.lv = lv;
  a.rule_facts(f);
  f.credited = tot[0];
  memcpy(f.sums, tot + 2, 32);
  f.accounts = npayee;
  const uint32_t k = claims.pay_accounts ? (uint32_t)std::min<uint64_t>(claims.npay, npayee) : 0;
  if (k) {
    DevBuf pa, ps, pf;
    uint32_t differs = qpk::LEDGER_AUDIT_NO_SEQ;
    QP_HIP_TRY(c, pa.alloc((size_t)k * 4));
    QP_HIP_TRY(c, ps.alloc((size_t)k * 4));
    QP_HIP_TRY(c, pf.alloc(k));
    QP_HIP_TRY(c, hipMemcpyAsync(pa.p, claims.pay_accounts, (size_t)k * 32, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(c, hipMemcpyAsync(ps.p, claims.pay_sums, (size_t)k * 32, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(c, hipMemcpyAsync(pf.p, claims.pay_first_seq, (size_t)k * 8, hipMemcpyHostToDevice, s));
    qpk::ledger_audit_payouts(d, payee, k, pa.p, ps.p, pf.p, rep, s);
    QP_HIP_TRY(c, hipGetLastError());
    QP_HIP_TRY(c, hipMemcpyAsync(&differs, &rep->payout, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(c, hipStreamSynchronize(s));
    if (differs != qpk::LEDGER_AUDIT_NO_SEQ) f.payout = differs;
  }
  // the prefix roots of the commitments that name a prefix, in one batch, once no earlier reason fired
  PrefixRootBatch roots{tree, e, s, claims.commit_ns, claims.ncommit, n};
  ql::audit_verdict(f, n, claims, [&roots](uint32_t i, uint64_t, uint64_t out[4]) { roots.get(i, out); }, r);
  return roots.rc;
}

int refuse(qp_ctx *c, const std::string &why) {
  qla::set_ledgerless_error(c, "qp_ledger_log_audit: " + why);
  return QP_ERR_ARG;
}

}  // namespace

extern "C" int qp_ledger_log_audit(qp_ctx *c, const uint64_t *nullifiers, const uint64_t *numbers,
                                   const uint32_t *amounts, const uint64_t *accounts, const uint8_t *flags, uint64_t n,
                                   const uint64_t *claimed_root, const uint64_t *claimed_totals,
                                   const uint64_t *pay_accounts, const uint64_t *pay_sums,
                                   const uint64_t *pay_first_seq, uint64_t npay, const uint64_t *commit_roots,
                                   const uint64_t *commit_ns, uint32_t ncommit, qp_ledger_audit_report *out) {
  if (!out) return QP_ERR_ARG;
  ql::AuditLog g;
  g.nullifiers = nullifiers, g.numbers = numbers, g.amounts = amounts, g.accounts = accounts, g.flags = flags, g.n = n;
  ql::AuditClaims claims;
  claims.root = claimed_root;
  claims.totals = claimed_totals;
  claims.pay_accounts = pay_accounts;
  claims.pay_sums = pay_sums;
  claims.pay_first_seq = pay_first_seq;
  claims.npay = npay;
  claims.commit_roots = commit_roots;
  claims.commit_ns = commit_ns;
  claims.ncommit = ncommit;
  const std::string why = ql::audit_refusal(g, claims);
  if (!why.empty()) return refuse(c, why);
  ql::AuditReport &r = *reinterpret_cast<ql::AuditReport *>(out);
  try {
    if (!c) {
      ql::audit_host(g, claims, r);
      return QP_OK;
    }
    const int rc = audit_device(c, g, claims, r);
    if (rc) qla::set_ledgerless_error(c, "qp_ledger_log_audit: " + c->err);
    return rc;
  } catch (const std::bad_alloc &) {
    qla::set_ledgerless_error(c, "qp_ledger_log_audit: out of host memory");
    return QP_ERR_OOM;
  }
}
