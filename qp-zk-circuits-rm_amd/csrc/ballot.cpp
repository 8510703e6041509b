// ballot.cpp — the qp_ballot_box_* entry points (qpgpu.h): voting proofs
// verified through the batch verifier, their public inputs screened on the
// host (ballot_table.h), each nullifier admitted once.  With a context the
// nullifier set and the tally live on the device (ballot.hip); without one the
// same semantics run on the host (qb::HostBox).  The log commitment (find,
// commit_log, receipts and the receipt check: ballot_log.h) is the box's
// LogCommit (log_commit.h), brought up to date on demand; a cast does not touch
// it.  The nullifier-set commitment (commit_set, set_proofs: nullifier_set.h) is the
// box's SetCommit (set_commit.h) over the counted entries, rebuilt on demand
// only.  roots_at answers from the log tree; restore reopens a box from a published
// log through the audit's passes (ballot_audit.h, ballot_audit.cpp) and keeps
// the table they built.  The refusals worded alike for the box and the transfer
// ledger are handle_common.h's; what is stated here is the box's own.
#include "../../include/qpgpu.h"
#include <string.h>
#include <algorithm>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>
#include "acc_tree.h"
#include "ballot_audit.h"
#include "ballot_audit_device.h"
#include "ballot_kernels.h"
#include "ballot_log.h"
#include "ballot_table.h"
#include "ctx.h"
#include "handle_common.h"
#include "log_commit.h"
#include "set_commit.h"
#include "verifier.h"

static_assert(sizeof(qp_ballot_result) == sizeof(qb::Result) && sizeof(qb::Result) == 24, "qp_ballot_result layout");
static_assert(QP_RECEIPT_OK == qb::RECEIPT_OK && QP_RECEIPT_SHAPE == qb::RECEIPT_SHAPE &&
                  QP_RECEIPT_ROOT == qb::RECEIPT_ROOT && QP_RECEIPT_NON_CANONICAL == qb::RECEIPT_NON_CANONICAL &&
                  QP_RECEIPT_NULL == qb::RECEIPT_NULL,
              "qp_receipt_status and ballot_log.h differ");
static_assert(QP_BALLOT_COUNTED == qb::COUNTED && QP_BALLOT_PROOF_REJECTED == qb::PROOF_REJECTED &&
                  QP_BALLOT_MALFORMED == qb::MALFORMED && QP_BALLOT_WRONG_PROPOSAL == qb::WRONG_PROPOSAL &&
                  QP_BALLOT_UNKNOWN_ROOT == qb::UNKNOWN_ROOT && QP_BALLOT_BAD_VOTE == qb::BAD_VOTE &&
                  QP_BALLOT_DOUBLE_VOTE == qb::DOUBLE_VOTE,
              "qp_ballot_status and ballot_table.h differ");

using namespace qph;
using qba::DeviceTables;

struct qp_ballot_box : qb::Words {
  static constexpr int BROKEN = QP_ERR_STATE;  // what a broken invariant returns (the ledger: QP_ERR_HIP)
  qp_ctx *ctx = nullptr;                       // null: the host path
  std::string err;
  bool dead = false;  // a device step failed part-way, or the defensive error word was set: no further casts
  qb::Screen screen;
  uint64_t cast = 0;
  qb::Packed pk;  // the batch in flight
  qb::HostBox host;
  // ---- device path
  uint64_t capacity = 0, count = 0, yes = 0, no = 0;  // yes / no: the device counters as of the last cast
  DeviceTables t;
  DevBuf d_stay, d_first, d_ctr, d_audit;  // per batch: slot stayed at [k] (u32), first [k]; counters; recount's four
  std::vector<uint64_t> h_first;
  TimingEvents<3> ev;  // upload start, upload end, resolve end of the last cast
  float ms[2] = {0, 0};
  LogCommit<qb::HostLog> lc;         // the log commitment, both paths
  SetCommit sc;                      // the nullifier-set commitment, both paths
  DevBuf d_q, d_seq, d_nul, d_flag;  // per find / entries_at batch (LOG_BATCH entries)
  uint64_t admitted() const { return ctx ? count : host.count(); }
  uint64_t cap() const { return ctx ? capacity : host.capacity; }
};

namespace {
// why the last qp_ballot_box_new (restore, log_audit) on this thread was refused
thread_local HandlelessError g_new_err;

int refuse_new(qp_ctx *c, const std::string &why) {
  g_new_err.set(c, "qp_ballot_box_new: " + why);
  return QP_ERR_ARG;
}
}  // namespace

void qba::set_boxless_error(qp_ctx *c, const std::string &why) { g_new_err.set(c, why); }

namespace {
// the device steps of one batch: the packed ballots into log [count, count + k), insert, resolve
int cast_device(qp_ballot_box *b, qb::Result *out) {
  qp_ctx *c = b->ctx;
  const qb::Packed &pk = b->pk;
  const uint32_t k = (uint32_t)pk.size();
  hipStream_t s = c->stream;
  QP_HIP_TRY(b, hipSetDevice(c->device));
  for (hipEvent_t &e : b->ev.e)
    if (!e) QP_HIP_TRY(b, hipEventCreate(&e));
  if (b->d_first.words < k) {
    QP_HIP_TRY(b, b->d_stay.alloc(((size_t)k + 1) / 2));
    QP_HIP_TRY(b, b->d_first.alloc(k));
  }
  b->h_first.resize(k);
  const qpk::BallotDev d = b->t.dev();
  qpk::BallotCounters *ctr = b->d_ctr.as<qpk::BallotCounters>();
  qpk::BallotCounters now;
  QP_HIP_TRY(b, hipEventRecord(b->ev.e[0], s));
  QP_HIP_TRY(b, hipMemcpyAsync(d.nullifier + b->count * 4, pk.nullifier.data(), (size_t)k * 32, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(b, hipMemcpyAsync(d.number + b->count, pk.number.data(), (size_t)k * 8, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(b, hipMemcpyAsync(d.flags + b->count, pk.flags.data(), k, hipMemcpyHostToDevice, s));
  QP_HIP_TRY(b, hipEventRecord(b->ev.e[1], s));
  qpk::ballot_insert(d, (uint32_t)b->count, k, b->d_stay.as<uint32_t>(), ctr, s);
  QP_HIP_TRY(b, hipGetLastError());
  qpk::ballot_resolve(d, (uint32_t)b->count, k, b->d_stay.as<uint32_t>(), b->d_first.p, ctr, s);
  QP_HIP_TRY(b, hipGetLastError());
  QP_HIP_TRY(b, hipEventRecord(b->ev.e[2], s));
  QP_HIP_TRY(b, hipMemcpyAsync(b->h_first.data(), b->d_first.p, (size_t)k * 8, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(b, hipMemcpyAsync(&now, ctr, sizeof now, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(b, hipStreamSynchronize(s));
  QP_HIP_TRY(b, hipEventElapsedTime(&b->ms[0], b->ev.e[0], b->ev.e[1]));
  QP_HIP_TRY(b, hipEventElapsedTime(&b->ms[1], b->ev.e[1], b->ev.e[2]));
  if (now.err)
    return refuse(b, b->BROKEN, "qp_ballot_box_cast: the nullifier table's probe found no slot (an internal invariant broke)");
  for (uint32_t j = 0; j < k; j++) {
    qb::Result &r = out[pk.pos[j]];
    r.first = b->h_first[j];
    if (r.first != r.number) r.status = qb::DOUBLE_VOTE;
  }
  b->count += k;
  b->yes = now.yes;
  b->no = now.no;
  return QP_OK;
}

// pis [n][13], verdicts (may be null): screen, pack, refuse an overflow, count
int cast_screened(qp_ballot_box *b, const char *fn, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                  qb::Result *out) {
  qb::screen_and_pack(b->screen, pis, verdicts, n, b->cast, out, b->pk);
  const uint64_t k = b->pk.size();
  if (k > b->cap() - b->admitted()) return over_capacity(b, fn, k);
  if (!b->ctx) {
    b->host.admit_packed(b->pk, out);
  } else if (k) {
    const int rc = cast_device(b, out);
    if (rc) {
      b->dead = true;
      return rc;
    }
  }
  b->cast += n;
  return QP_OK;
}

// entries per k_ballot_find / k_ballot_gather launch (the batch buffers hold this many)
constexpr uint32_t LOG_BATCH = 8192;

int log_batch_buffers(qp_ballot_box *b) {
  if (b->d_q.p) return QP_OK;
  QP_HIP_TRY(b, b->d_seq.alloc(LOG_BATCH));
  QP_HIP_TRY(b, b->d_nul.alloc((size_t)LOG_BATCH * 4));
  QP_HIP_TRY(b, b->d_flag.alloc(LOG_BATCH / 8));
  QP_HIP_TRY(b, b->d_q.alloc((size_t)LOG_BATCH * 4));
  return QP_OK;
}

// the defensive error word after a launch of the log's kernels (copied by the caller, stream synchronised)
int log_error_word(qp_ballot_box *b, const char *fn, uint32_t err) {
  if (!err) return QP_OK;
  return refuse(b, b->BROKEN, std::string(fn) + (err & 4 ? ": a ballot number in the log is not a field element"
                                                         : ": a slot of the nullifier table holds no log entry") +
                                  " (an internal invariant broke)");
}

int find_device(qp_ballot_box *b, const uint64_t *nullifiers, uint32_t k, uint64_t *seq_out) {
  qp_ctx *c = b->ctx;
  hipStream_t s = c->stream;
  QP_HIP_TRY(b, hipSetDevice(c->device));
  int rc = log_batch_buffers(b);
  if (rc) return rc;
  qpk::BallotCounters *ctr = b->d_ctr.as<qpk::BallotCounters>();
  std::vector<uint32_t> h(std::min(k, LOG_BATCH));
  uint32_t err = 0;
  for (uint32_t done = 0; done < k;) {
    const uint32_t nb = std::min(LOG_BATCH, k - done);
    QP_HIP_TRY(b, hipMemcpyAsync(b->d_q.p, nullifiers + (size_t)done * 4, (size_t)nb * 32, hipMemcpyHostToDevice, s));
    qpk::ballot_find(b->t.dev(), (uint32_t)b->count, b->d_q.p, nb, b->d_seq.as<uint32_t>(), ctr, s);
    QP_HIP_TRY(b, hipGetLastError());
    QP_HIP_TRY(b, hipMemcpyAsync(h.data(), b->d_seq.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(b, hipMemcpyAsync(&err, &ctr->err, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(b, hipStreamSynchronize(s));
    if ((rc = log_error_word(b, "qp_ballot_box_find", err))) return rc;
    for (uint32_t i = 0; i < nb; i++) seq_out[done + i] = h[i] == qb::EMPTY ? qb::NOT_FOUND : h[i];
    done += nb;
  }
  return QP_OK;
}

// the log commitment up to the admitted count (> 0; the caller checks), on either path
int commit(qp_ballot_box *b) {
  const char *fn = "qp_ballot_box_commit_log";
  if (!b->ctx) return b->lc.commit(b->host) ? QP_OK : log_error_word(b, fn, 4);
  qpk::BallotCounters *ctr = b->d_ctr.as<qpk::BallotCounters>();
  auto leaves = [&](uint32_t first, uint32_t end, uint64_t *dig) {
    qpk::ballot_leaves(b->t.dev(), first, end, dig, ctr, b->ctx->stream);
  };
  uint32_t word = 0;
  if (int rc = b->lc.commit(b->ctx, b->err, fn, b->BROKEN, b->count, b->capacity, leaves, &ctr->err, &word)) return rc;
  return log_error_word(b, fn, word);
}

// the set commitment over the counted entries of the log as it stands, on either path.  A box's log
// never counts one nullifier twice: a duplicate member is the defensive error.
int commit_members(qp_ballot_box *b, const char *fn) {
  uint64_t dup = qb::NOT_FOUND;
  if (!b->ctx) {
    b->sc.commit_host(b->host.nullifier.data(), b->host.flags.data(), b->host.count(), qb::FLAG_COUNTED, &dup);
  } else {
    const qpk::BallotDev d = b->t.dev();
    if (int rc = b->sc.commit_device(b->ctx, b->err, d.nullifier, d.flags, b->count, qb::FLAG_COUNTED, &dup)) {
      b->err = std::string(fn) + ": " + b->err;
      return rc;
    }
  }
  if (dup == qb::NOT_FOUND) return QP_OK;
  b->dead = true;
  return refuse(b, b->BROKEN, std::string(fn) + ": entry " + std::to_string(dup) +
                                  " is counted and an earlier counted entry has its nullifier (an internal invariant broke)");
}

int entries_at_device(qp_ballot_box *b, const uint64_t *seqs, uint32_t k, uint64_t *nullifiers, uint64_t *numbers,
                      uint8_t *flags) {
  qp_ctx *c = b->ctx;
  hipStream_t s = c->stream;
  QP_HIP_TRY(b, hipSetDevice(c->device));
  const int rc = log_batch_buffers(b);
  if (rc) return rc;
  for (uint32_t done = 0; done < k;) {
    const uint32_t nb = std::min(LOG_BATCH, k - done);
    QP_HIP_TRY(b, hipMemcpyAsync(b->d_q.p, seqs + done, (size_t)nb * 8, hipMemcpyHostToDevice, s));
    qpk::ballot_gather(b->t.dev(), b->d_q.p, nb, b->d_nul.p, b->d_seq.p, b->d_flag.as<uint8_t>(), s);
    QP_HIP_TRY(b, hipGetLastError());
    if (nullifiers)
      QP_HIP_TRY(b, hipMemcpyAsync(nullifiers + (size_t)done * 4, b->d_nul.p, (size_t)nb * 32, hipMemcpyDeviceToHost, s));
    if (numbers) QP_HIP_TRY(b, hipMemcpyAsync(numbers + done, b->d_seq.p, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    if (flags) QP_HIP_TRY(b, hipMemcpyAsync(flags + done, b->d_flag.p, nb, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(b, hipStreamSynchronize(s));
    done += nb;
  }
  return QP_OK;
}

}  // namespace

extern "C" {

int qp_ballot_box_new(qp_ctx *c, const uint64_t proposal_id[4], const uint64_t *roots, uint32_t nroots,
                      uint64_t capacity, qp_ballot_box **out) {
  if (!out) return QP_ERR_ARG;
  *out = nullptr;
  if (!proposal_id || !roots) return refuse_new(c, "null proposal_id or roots");
  if (!qb::canonical(proposal_id, 4)) return refuse_new(c, "proposal_id is not four canonical field elements");
  if (!nroots || nroots > qb::MAX_ROOTS)
    return refuse_new(c, std::to_string(nroots) + " accepted roots: a box needs 1 to " + std::to_string(qb::MAX_ROOTS));
  if (!qb::canonical(roots, nroots * 4)) return refuse_new(c, "a root is not four canonical field elements");
  if (!capacity || capacity > qb::MAX_CAPACITY)
    return refuse_new(c, "capacity " + std::to_string(capacity) + ": it must be 1 to 2^31 admitted ballots");
  std::unique_ptr<qp_ballot_box> b(new (std::nothrow) qp_ballot_box);
  if (!b) return QP_ERR_OOM;
  b->ctx = c;
  memcpy(b->screen.proposal, proposal_id, 32);
  try {
    for (uint32_t i = 0; i < nroots; i++)
      if (!b->screen.has_root(roots + 4 * i)) b->screen.roots.insert(b->screen.roots.end(), roots + 4 * i, roots + 4 * i + 4);
    if (!c) {
      b->host.open(capacity);
      *out = b.release();
      return QP_OK;
    }
  } catch (const std::bad_alloc &) {
    g_new_err.text = "qp_ballot_box_new: out of host memory";
    return QP_ERR_OOM;
  }
  int rc = QP_OK;
  auto device_open = [&]() -> int {
    QP_HIP_TRY(b, hipSetDevice(c->device));
    if ((rc = qba::alloc_tables({b->err}, c->stream, capacity, b->t))) return rc;
    QP_HIP_TRY(b, b->d_ctr.alloc((sizeof(qpk::BallotCounters) + 7) / 8));
    QP_HIP_TRY(b, b->d_audit.alloc(4));
    QP_HIP_TRY(b, hipMemsetAsync(b->d_ctr.p, 0, sizeof(qpk::BallotCounters), c->stream));
    QP_HIP_TRY(b, hipStreamSynchronize(c->stream));
    return QP_OK;
  };
  if ((rc = device_open())) {
    g_new_err.set(c, "qp_ballot_box_new: " + b->err);
    return rc;
  }
  b->capacity = capacity;
  *out = b.release();
  return QP_OK;
}

void qp_ballot_box_free(qp_ballot_box *b) {
  if (!b) return;
  if (b->ctx) (void)hipSetDevice(b->ctx->device);
  delete b;
}

const char *qp_ballot_box_last_error(const qp_ballot_box *b) { return b ? b->err.c_str() : g_new_err.text.c_str(); }

int qp_ballot_box_accept_root(qp_ballot_box *b, const uint64_t root[4]) {
  if (!b) return QP_ERR_ARG;
  if (!root || !qb::canonical(root, 4)) {
    b->err = "qp_ballot_box_accept_root: the root must be four canonical field elements";
    return QP_ERR_ARG;
  }
  if (b->screen.has_root(root)) return QP_OK;
  if (b->screen.roots.size() / 4 >= qb::MAX_ROOTS) {
    b->err = "qp_ballot_box_accept_root: the box already accepts " + std::to_string(qb::MAX_ROOTS) + " roots, the most";
    return QP_ERR_ARG;
  }
  try {
    b->screen.roots.insert(b->screen.roots.end(), root, root + 4);
  } catch (const std::bad_alloc &) {
    return bad_alloc(b, "qp_ballot_box_accept_root");
  }
  return QP_OK;
}

int qp_ballot_box_cast_public(qp_ballot_box *b, const uint64_t *pis, const uint32_t *verdicts, uint32_t n,
                              qp_ballot_result *out) {
  if (!b) return QP_ERR_ARG;
  if (b->dead) return dead_handle(b, "qp_ballot_box_cast_public");
  if (!n) return QP_OK;
  if (!pis || !out) return null_buffer(b, "qp_ballot_box_cast_public");
  try {
    return cast_screened(b, "qp_ballot_box_cast_public", pis, verdicts, n, reinterpret_cast<qb::Result *>(out));
  } catch (const std::bad_alloc &) {
    return bad_alloc(b, "qp_ballot_box_cast_public");
  }
}

int qp_ballot_box_cast(qp_ballot_box *b, struct qp_verifier *v, const uint8_t *const *proofs, const size_t *lens,
                       uint32_t n, qp_ballot_result *out) {
  if (!b) return QP_ERR_ARG;
  if (b->dead) return dead_handle(b, "qp_ballot_box_cast");
  if (int rc = check_verifier(b, "qp_ballot_box_cast", v, qb::NPI, "a voting circuit's")) return rc;
  if (!n) return QP_OK;
  if (!proofs || !lens || !out) return null_buffer(b, "qp_ballot_box_cast");
  try {
    std::vector<uint32_t> verdicts;
    std::vector<uint64_t> pis;
    if (int rc = verify_and_gather(b, "qp_ballot_box_cast", v, proofs, lens, n, qb::NPI, verdicts, pis)) return rc;
    return cast_screened(b, "qp_ballot_box_cast", pis.data(), verdicts.data(), n, reinterpret_cast<qb::Result *>(out));
  } catch (const std::bad_alloc &) {
    return bad_alloc(b, "qp_ballot_box_cast");
  }
}

int qp_ballot_box_reserve(qp_ballot_box *b, uint64_t new_capacity) {
  if (!b) return QP_ERR_ARG;
  if (b->dead) return dead_handle(b, "qp_ballot_box_reserve");
  if (int rc = check_reserve(b, "qp_ballot_box_reserve", new_capacity)) return rc;
  if (new_capacity == b->cap()) return QP_OK;
  if (!b->ctx) {
    try {
      b->host.reserve(new_capacity);
    } catch (const std::bad_alloc &) {
      return bad_alloc(b, "qp_ballot_box_reserve");
    }
    b->lc.drop();
    return QP_OK;
  }
  // a new log and table beside the old; the box moves over only once all of it succeeded
  qp_ctx *c = b->ctx;
  hipStream_t s = c->stream;
  DeviceTables nt;
  qpk::BallotCounters now;
  QP_HIP_TRY(b, hipSetDevice(c->device));
  const int rc = qba::alloc_tables({b->err}, s, new_capacity, nt);
  if (rc) return rc;
  const qpk::BallotDev od = b->t.dev(), nd = nt.dev();
  qpk::BallotCounters *ctr = b->d_ctr.as<qpk::BallotCounters>();
  if (b->count) {
    QP_HIP_TRY(b, hipMemcpyAsync(nd.nullifier, od.nullifier, b->count * 32, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(b, hipMemcpyAsync(nd.number, od.number, b->count * 8, hipMemcpyDeviceToDevice, s));
    QP_HIP_TRY(b, hipMemcpyAsync(nd.flags, od.flags, b->count, hipMemcpyDeviceToDevice, s));
    qpk::ballot_rebuild(nd, (uint32_t)b->count, ctr, s);
    QP_HIP_TRY(b, hipGetLastError());
  }
  QP_HIP_TRY(b, hipMemcpyAsync(&now, ctr, sizeof now, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(b, hipStreamSynchronize(s));
  if (now.err)
    return device_step(b, refuse(b, b->BROKEN, "qp_ballot_box_reserve: the nullifier table's probe found no slot (an internal "
                                               "invariant broke)"));
  b->t = std::move(nt);
  b->capacity = new_capacity;
  b->lc.drop();
  return QP_OK;
}

int qp_ballot_box_tally(const qp_ballot_box *b, uint64_t *yes, uint64_t *no) {
  if (!b) return QP_ERR_ARG;
  if (yes) *yes = b->ctx ? b->yes : b->host.yes;
  if (no) *no = b->ctx ? b->no : b->host.no;
  return QP_OK;
}

int qp_ballot_box_state(const qp_ballot_box *b, uint64_t *cast, uint64_t *admitted, uint64_t *capacity) {
  if (!b) return QP_ERR_ARG;
  if (cast) *cast = b->cast;
  if (admitted) *admitted = b->admitted();
  if (capacity) *capacity = b->cap();
  return QP_OK;
}

int qp_ballot_box_entries(qp_ballot_box *b, uint64_t first, uint64_t k, uint64_t *nullifiers, uint64_t *numbers,
                          uint8_t *flags) {
  if (!b) return QP_ERR_ARG;
  if (int rc = check_range(b, "qp_ballot_box_entries", first, k)) return rc;
  if (!k) return QP_OK;
  if (!b->ctx) {
    if (nullifiers) memcpy(nullifiers, &b->host.nullifier[first * 4], k * 32);
    if (numbers) memcpy(numbers, &b->host.number[first], k * 8);
    if (flags) memcpy(flags, &b->host.flags[first], k);
    return QP_OK;
  }
  qp_ctx *c = b->ctx;
  hipStream_t s = c->stream;
  const qpk::BallotDev d = b->t.dev();
  QP_HIP_TRY(b, hipSetDevice(c->device));
  if (nullifiers) QP_HIP_TRY(b, hipMemcpyAsync(nullifiers, d.nullifier + first * 4, k * 32, hipMemcpyDeviceToHost, s));
  if (numbers) QP_HIP_TRY(b, hipMemcpyAsync(numbers, d.number + first, k * 8, hipMemcpyDeviceToHost, s));
  if (flags) QP_HIP_TRY(b, hipMemcpyAsync(flags, d.flags + first, k, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(b, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_ballot_box_recount(qp_ballot_box *b, uint64_t out[4]) {
  if (!b || !out) return QP_ERR_ARG;
  if (!b->ctx) {
    b->host.recount(out);
    return QP_OK;
  }
  qp_ctx *c = b->ctx;
  hipStream_t s = c->stream;
  QP_HIP_TRY(b, hipSetDevice(c->device));
  QP_HIP_TRY(b, hipMemsetAsync(b->d_audit.p, 0, 32, s));
  qpk::ballot_recount(b->t.flags.as<uint8_t>(), (uint32_t)b->count, b->d_audit.as<unsigned long long>(), s);
  QP_HIP_TRY(b, hipGetLastError());
  QP_HIP_TRY(b, hipMemcpyAsync(out, b->d_audit.p, 32, hipMemcpyDeviceToHost, s));
  QP_HIP_TRY(b, hipStreamSynchronize(s));
  return QP_OK;
}

int qp_ballot_box_find(qp_ballot_box *b, const uint64_t *nullifiers, uint32_t k, uint64_t *seq_out) {
  if (!b) return QP_ERR_ARG;
  if (b->dead) return dead_handle(b, "qp_ballot_box_find");
  if (!k) return QP_OK;
  if (!nullifiers || !seq_out) return null_buffer(b, "qp_ballot_box_find");
  if (int rc = canonical_keys(b, "qp_ballot_box_find", "nullifier", nullifiers, k)) return rc;
  if (!b->ctx) {
    for (uint32_t i = 0; i < k; i++) seq_out[i] = b->host.find(nullifiers + (size_t)i * 4);
    return QP_OK;
  }
  try {
    return device_step(b, find_device(b, nullifiers, k, seq_out));
  } catch (const std::bad_alloc &) {
    return bad_alloc(b, "qp_ballot_box_find");
  }
}

int qp_ballot_box_commit_log(qp_ballot_box *b, uint64_t root_out[4], uint64_t *n_out) {
  return qph::commit_log(b, "qp_ballot_box_commit_log", commit, root_out, n_out);
}

int qp_ballot_box_receipts(qp_ballot_box *b, const uint64_t *seqs, uint32_t k, uint64_t *siblings, uint32_t *path_bits,
                           uint32_t *depth, uint64_t *leaves, uint64_t root_out[4], uint64_t *n_out) {
  return qph::receipts(b, "qp_ballot_box_receipts", commit, seqs, k, siblings, path_bits, depth, leaves, root_out, n_out);
}

int qp_ballot_box_entries_at(qp_ballot_box *b, const uint64_t *seqs, uint32_t k, uint64_t *nullifiers,
                             uint64_t *numbers, uint8_t *flags) {
  if (!b) return QP_ERR_ARG;
  if (b->dead) return dead_handle(b, "qp_ballot_box_entries_at");
  if (!k) return QP_OK;
  if (!seqs) return null_buffer(b, "qp_ballot_box_entries_at");
  const int rc = check_seqs(b, "qp_ballot_box_entries_at", seqs, k);
  if (rc) return rc;
  if (b->ctx) return device_step(b, entries_at_device(b, seqs, k, nullifiers, numbers, flags));
  for (uint32_t i = 0; i < k; i++) {
    if (nullifiers) memcpy(nullifiers + (size_t)i * 4, &b->host.nullifier[seqs[i] * 4], 32);
    if (numbers) numbers[i] = b->host.number[seqs[i]];
    if (flags) flags[i] = b->host.flags[seqs[i]];
  }
  return QP_OK;
}

int qp_ballot_box_roots_at(qp_ballot_box *b, const uint64_t *ms, uint32_t k, uint64_t *roots_out) {
  return qph::roots_at(b, "qp_ballot_box_roots_at", commit, qb::log_node, ms, k, roots_out);
}

int qp_ballot_box_restore(qp_ctx *c, const uint64_t proposal_id[4], const uint64_t *roots, uint32_t nroots,
                          uint64_t capacity, const uint64_t *nullifiers, const uint64_t *numbers, const uint8_t *flags,
                          uint64_t n, uint64_t cast_count, const uint64_t *expect_root, qp_ballot_box **out) {
  if (!out) return QP_ERR_ARG;
  *out = nullptr;
  auto refuse = [c](int rc, const std::string &why) {
    qba::set_boxless_error(c, "qp_ballot_box_restore: " + why);
    return rc;
  };
  if (n && (!nullifiers || !numbers || !flags)) return refuse(QP_ERR_ARG, "null log buffer");
  if (expect_root && (!n || !qb::canonical(expect_root, 4)))
    return refuse(QP_ERR_ARG, n ? "the expected root is not four canonical field elements" : "an empty log has no root");
  try {
    const std::string why = qb::restore_refusal(numbers, n, capacity, cast_count);
    if (!why.empty()) return refuse(QP_ERR_ARG, why);
    qp_ballot_box *fresh = nullptr;
    int rc = qp_ballot_box_new(c, proposal_id, roots, nroots, capacity, &fresh);
    if (rc) return rc;  // qp_ballot_box_new left its reason
    std::unique_ptr<qp_ballot_box, void (*)(qp_ballot_box *)> b(fresh, qp_ballot_box_free);
    b->cast = cast_count;
    if (!n) {
      *out = b.release();
      return QP_OK;
    }
    qb::AuditFacts f;
    bool canonical = false;
    if (!c) {
      qb::HostLog tree;
      canonical = qb::audit_facts_host(nullifiers, numbers, flags, n, capacity, expect_root != nullptr, b->host, tree, f);
    } else {
      // the log into the new box's own buffers and its fresh table: what the audit builds is what the box keeps
      hipStream_t s = c->stream;
      const qpk::BallotDev d = b->t.dev();
      // With an expected root the audit builds the log tree for n leaves in `tree`, and the tree is discarded
      // on purpose: a restored box has committed nothing yet, and its own tree is laid out for the capacity,
      // not for n, by the first commit_log (which hashes these leaves again).  qp_ledger_restore instead
      // commits the restored ledger's own tree and keeps it; the two are left as they are, since making
      // them one changes what a commit_log after a restore launches.
      AccTree tree;
      auto device_restore = [&]() -> int {
        QP_HIP_TRY(b, hipSetDevice(c->device));
        QP_HIP_TRY(b, hipMemcpyAsync(d.nullifier, nullifiers, (size_t)n * 32, hipMemcpyHostToDevice, s));
        QP_HIP_TRY(b, hipMemcpyAsync(d.number, numbers, (size_t)n * 8, hipMemcpyHostToDevice, s));
        QP_HIP_TRY(b, hipMemcpyAsync(d.flags, flags, (size_t)n, hipMemcpyHostToDevice, s));
        if (int r = qba::audit_facts_device(c, {b->err}, d, n, expect_root ? &tree : nullptr, f, &canonical)) return r;
        if (!canonical) return QP_OK;
        const qpk::BallotCounters now{f.yes, f.no, 0, 0};
        QP_HIP_TRY(b, hipMemcpyAsync(b->d_ctr.p, &now, sizeof now, hipMemcpyHostToDevice, s));
        QP_HIP_TRY(b, hipStreamSynchronize(s));
        return QP_OK;
      };
      if ((rc = device_restore())) return refuse(rc, b->err);
      b->count = n;
      b->yes = f.yes;
      b->no = f.no;
    }
    qb::AuditReport r;
    if (!canonical) {
      qb::audit_non_canonical(f.non_canonical, r);
    } else {
      qb::AuditClaims claims;
      claims.root = expect_root;
      qb::audit_verdict(f, n, claims, qb::AUDIT_RESTORE_REASONS, [](uint32_t, uint64_t, uint64_t *) {}, r);
    }
    if (r.status != qb::AUDIT_OK) return refuse(QP_ERR_FORMAT, qb::audit_failure_text(r));
    *out = b.release();
    return QP_OK;
  } catch (const std::bad_alloc &) {
    return refuse(QP_ERR_OOM, "out of host memory");
  }
}

int qp_ballot_receipt_check(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t nullifier[4],
                            uint64_t number, uint8_t flags, const uint64_t *siblings, uint32_t path_bits,
                            uint32_t depth) {
  if (!root || !nullifier || !siblings) return QP_RECEIPT_NULL;
  return qb::receipt_check(root, n, seq, nullifier, number, flags, siblings, path_bits, depth);
}

int qp_ballot_box_commit_set(qp_ballot_box *b, uint64_t root_out[4], uint64_t *m_out) {
  return qph::commit_set(b, "qp_ballot_box_commit_set", commit_members, root_out, m_out);
}

int qp_ballot_box_set_proofs(qp_ballot_box *b, const uint64_t *keys, uint32_t k, uint8_t *found, uint64_t *pos,
                             uint64_t *lo_key, uint64_t *lo_seq, uint64_t *lo_siblings, uint32_t *lo_bits,
                             uint32_t *lo_depth, uint64_t *hi_key, uint64_t *hi_seq, uint64_t *hi_siblings,
                             uint32_t *hi_bits, uint32_t *hi_depth, uint64_t root_out[4], uint64_t *m_out) {
  const SetCommit::Out o{found, pos, {lo_key, hi_key}, {lo_seq, hi_seq}, {lo_siblings, hi_siblings}, {lo_bits, hi_bits},
                         {lo_depth, hi_depth}};
  return qph::set_proofs(b, "qp_ballot_box_set_proofs", commit_members, keys, k, o, root_out, m_out);
}

int qp_ballot_box_cast_times(const qp_ballot_box *b, double ms[2]) {
  if (!b || !ms) return QP_ERR_ARG;
  ms[0] = b->ms[0];
  ms[1] = b->ms[1];
  return QP_OK;
}

}  // extern "C"
