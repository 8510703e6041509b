// ballot_audit.cpp — qp_ballot_log_audit (qpgpu.h), and the device path of the
// audit that it and qp_ballot_box_restore (ballot.cpp) share.  An audit needs no
// box: with a context the log is uploaded into tables of this call's own
// (ballot_audit_device.h's DeviceTables), the fresh table takes it whole, the
// tree is log_commit.h's whole-log form, and the verdict is ballot_audit.h's,
// the same the host path reaches.
#include "../../include/qpgpu.h"
#include <string.h>
#include <new>
#include <string>
#include <vector>
#include "ballot_audit.h"
#include "ballot_audit_device.h"
#include "log_commit.h"

static_assert(sizeof(qp_audit_report) == sizeof(qb::AuditReport) && sizeof(qb::AuditReport) == 80, "qp_audit_report layout");
static_assert(QP_AUDIT_OK == qb::AUDIT_OK && QP_AUDIT_NON_CANONICAL == qb::AUDIT_NON_CANONICAL &&
                  QP_AUDIT_ORDER == qb::AUDIT_ORDER && QP_AUDIT_COUNT_RULE == qb::AUDIT_COUNT_RULE &&
                  QP_AUDIT_TALLY == qb::AUDIT_TALLY && QP_AUDIT_ROOT == qb::AUDIT_ROOT &&
                  QP_AUDIT_COMMITMENT == qb::AUDIT_COMMITMENT,
              "qp_audit_status and ballot_audit.h differ");

namespace qba {

int audit_facts_device(qp_ctx *c, AccErr e, const qpk::BallotDev &d, uint64_t n, AccTree *tree, qb::AuditFacts &f,
                       bool *canonical) {
  hipStream_t s = c->stream;
  f = qb::AuditFacts();
  *canonical = false;
  DevBuf d_rep, d_stay;
  QP_HIP_TRY(&e, d_rep.alloc((sizeof(qpk::BallotAuditDev) + 7) / 8));
  QP_HIP_TRY(&e, d_stay.alloc((size_t)((n + 1) / 2)));
  qpk::BallotAuditDev *rep = d_rep.as<qpk::BallotAuditDev>();
  qpk::BallotAuditDev h;
  memset(&h, 0, sizeof h);
  h.count_rule = ~0ull;
  h.non_canonical = h.order = qpk::AUDIT_NO_SEQ;
  QP_HIP_TRY(&e, hipMemcpyAsync(rep, &h, sizeof h, hipMemcpyHostToDevice, s));
  qpk::ballot_audit_screen(d, (uint32_t)n, rep, s);
  QP_HIP_TRY(&e, hipGetLastError());
  QP_HIP_TRY(&e, hipMemcpyAsync(&h, rep, sizeof h, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(&e, hipStreamSynchronize(s));
  if (h.non_canonical != qpk::AUDIT_NO_SEQ) {
    f.non_canonical = h.non_canonical;
    return QP_OK;
  }
  qpk::ballot_insert(d, 0, (uint32_t)n, d_stay.as<uint32_t>(), &rep->ctr, s);
  QP_HIP_TRY(&e, hipGetLastError());
  qpk::ballot_audit_resolve(d, (uint32_t)n, d_stay.as<uint32_t>(), rep, s);
  QP_HIP_TRY(&e, hipGetLastError());
  qpk::AccLevels lv;
  if (tree) {
    auto leaves = [&](uint32_t first, uint32_t end, uint64_t *dig) { qpk::ballot_leaves(d, first, end, dig, &rep->ctr, s); };
    if (int rc = log_tree_whole(e, s, *tree, n, leaves, lv, f.root)) return rc;
  }
  QP_HIP_TRY(&e, hipMemcpyAsync(&h, rep, sizeof h, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(&e, hipStreamSynchronize(s));
  if (h.ctr.err) {
    // bit 0: k_ballot_insert; bit 1: k_audit_resolve; bit 2: k_ballot_leaves (cannot be reached after the screen)
    e.err = std::string(h.ctr.err & 1   ? "the nullifier table's probe found no slot"
                        : h.ctr.err & 4 ? "a ballot number in the log is not a field element"
                                        : "a slot of the nullifier table does not hold its nullifier's first entry") +
            " (an internal invariant broke)";
    return QP_ERR_STATE;
  }
  if (tree) tree->lv = lv;
  if (h.order != qpk::AUDIT_NO_SEQ) f.order = h.order;
  if (h.count_rule != ~0ull) {
    f.count_rule = h.count_rule >> 32;
    f.first = h.count_rule & 0xFFFFFFFFu;
  }
  f.yes = h.ctr.yes;
  f.no = h.ctr.no;
  f.counted = h.counted;
  *canonical = true;
  return QP_OK;
}

}  // namespace qba

namespace {

int audit_device(qp_ctx *c, const uint64_t *nullifiers, const uint64_t *numbers, const uint8_t *flags, uint64_t n,
                 const qb::AuditClaims &claims, qb::AuditReport &r) {
  hipStream_t s = c->stream;
  AccErr e{c->err};
  QP_HIP_TRY(c, hipSetDevice(c->device));
  qba::DeviceTables t;
  if (int rc = qba::alloc_tables(e, s, n, t)) return rc;
  const qpk::BallotDev d = t.dev();
  QP_HIP_TRY(c, hipMemcpyAsync(d.nullifier, nullifiers, (size_t)n * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipMemcpyAsync(d.number, numbers, (size_t)n * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(c, hipMemcpyAsync(d.flags, flags, (size_t)n, hipMemcpyHostToDevice, s));
  AccTree tree;
  qb::AuditFacts f;
  bool canonical = false;
  int rc = qba::audit_facts_device(c, e, d, n, &tree, f, &canonical);
  if (rc) return rc;
  if (!canonical) {
    qb::audit_non_canonical(f.non_canonical, r);
    return QP_OK;
  }
  // the prefix roots of the commitments that name a prefix, in one batch, once no earlier reason fired
  PrefixRootBatch roots{tree, e, s, claims.commit_ns, claims.ncommit, n};
  qb::audit_verdict(f, n, claims, qb::AUDIT_ALL_REASONS, [&roots](uint32_t i, uint64_t, uint64_t out[4]) { roots.get(i, out); }, r);
  return roots.rc;
}

int refuse(qp_ctx *c, const std::string &why) {
  qba::set_boxless_error(c, "qp_ballot_log_audit: " + why);
  return QP_ERR_ARG;
}

}  // namespace

extern "C" int qp_ballot_log_audit(qp_ctx *c, const uint64_t *nullifiers, const uint64_t *numbers, const uint8_t *flags,
                                   uint64_t n, const uint64_t *claimed_root, const uint64_t *claimed_tally,
                                   const uint64_t *commit_roots, const uint64_t *commit_ns, uint32_t ncommit,
                                   qp_audit_report *out) {
  if (!out) return QP_ERR_ARG;
  if (!nullifiers || !numbers || !flags) return refuse(c, "null buffer");
  qb::AuditClaims claims;
  claims.root = claimed_root;
  claims.tally = claimed_tally;
  claims.commit_roots = commit_roots;
  claims.commit_ns = commit_ns;
  claims.ncommit = ncommit;
  const std::string why = qb::audit_refusal(n, claims);
  if (!why.empty()) return refuse(c, why);
  qb::AuditReport &r = *reinterpret_cast<qb::AuditReport *>(out);
  try {
    if (!c) {
      qb::audit_host(nullifiers, numbers, flags, n, claims, qb::AUDIT_ALL_REASONS, r);
      return QP_OK;
    }
    const int rc = audit_device(c, nullifiers, numbers, flags, n, claims, r);
    if (rc) qba::set_boxless_error(c, "qp_ballot_log_audit: " + c->err);
    return rc;
  } catch (const std::bad_alloc &) {
    qba::set_boxless_error(c, "qp_ballot_log_audit: out of host memory");
    return QP_ERR_OOM;
  }
}
