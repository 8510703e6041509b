// nullifier_set.cpp — the qp_nullifier_set_* entry points (qpgpu.h) that need
// no handle: the set commitment of a published log on either path (a SetCommit
// of the call's own, set_commit.h), the checker of a membership / absence proof
// (nullifier_set.h; host only), the sort's tile size and the stage times of the
// last device build.  The handles' calls are in ballot.cpp and ledger.cpp.
#include "../../include/qpgpu.h"
#include <string.h>
#include <new>
#include <string>
#include <vector>
#include "ctx.h"
#include "nullifier_set.h"
#include "set_commit.h"

static_assert(QP_SET_ORDER == qns::SET_ORDER && QP_RECEIPT_OK == qns::RECEIPT_OK, "qp_set_status and nullifier_set.h differ");

namespace {
thread_local std::string g_err;

int refuse(qp_ctx *c, int rc, const std::string &why) {
  g_err = "qp_nullifier_set_root: " + why;
  if (c) c->err = g_err;
  return rc;
}

int root_device(qp_ctx *c, SetCommit &sc, const uint64_t *nullifiers, const uint8_t *member, uint64_t n, uint64_t *order_out,
                uint64_t *dup) {
  std::string &err = c->err;
  AccErr e{err};
  hipStream_t s = c->stream;
  DevBuf d_nul, d_flags;
  QP_HIP_TRY(&e, hipSetDevice(c->device));
  if (n) {
    QP_HIP_TRY(&e, d_nul.alloc(n * 4));
    QP_HIP_TRY(&e, d_flags.alloc((n + 7) / 8));
    QP_HIP_TRY(&e, hipMemcpyAsync(d_nul.p, nullifiers, n * 32, hipMemcpyHostToDevice, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(d_flags.p, member, n, hipMemcpyHostToDevice, s));
  }
  if (int rc = sc.commit_device(c, err, d_nul.p, d_flags.as<uint8_t>(), n, 0xFF, dup)) return rc;
  if (order_out && sc.m) {
    std::vector<uint32_t> h(sc.m);
    QP_HIP_TRY(&e, hipMemcpyAsync(h.data(), sc.recs(sc.cur).seq, sc.m * 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    for (uint64_t j = 0; j < sc.m; j++) order_out[j] = h[j];
  }
  return QP_OK;
}
}  // namespace

extern "C" {

uint32_t qp_nullifier_set_tile(void) { return qpk::NSET_TILE; }

const char *qp_nullifier_set_last_error(void) { return g_err.c_str(); }

uint32_t qp_nullifier_set_times(double *ms, uint32_t cap) {
  const std::vector<double> &t = set_commit_last_times();
  if (!ms || cap < t.size()) return 0;
  for (size_t i = 0; i < t.size(); i++) ms[i] = t[i];
  return (uint32_t)t.size();
}

int qp_nullifier_set_root(qp_ctx *c, const uint64_t *nullifiers, const uint8_t *member, uint64_t n, uint64_t root_out[4],
                          uint64_t *m_out, uint64_t *order_out, uint64_t *dup_out) {
  if (n > qns::ACC_MAX_LEAVES) return refuse(c, QP_ERR_ARG, "a log of " + std::to_string(n) + " entries: the most is 2^31");
  if (n && (!nullifiers || !member)) return refuse(c, QP_ERR_ARG, "null log buffer");
  for (uint64_t seq = 0; seq < n; seq++)
    if (member[seq] && !qns::canonical(nullifiers + seq * 4, 4))
      return refuse(c, QP_ERR_ARG, "the nullifier of member entry " + std::to_string(seq) + " is not four canonical field elements");
  try {
    SetCommit sc;
    uint64_t dup = qns::NOT_FOUND;
    if (c) {
      if (int rc = root_device(c, sc, nullifiers, member, n, order_out, &dup)) return refuse(c, rc, c->err);
    } else {
      sc.commit_host(nullifiers, member, n, 0xFF, &dup);
      if (order_out)
        for (uint64_t j = 0; j < sc.m; j++) order_out[j] = sc.hset.seqs[j];
    }
    sc.pair(root_out, m_out);
    if (dup_out) *dup_out = dup;
    return QP_OK;
  } catch (const std::bad_alloc &) {
    return refuse(c, QP_ERR_OOM, "out of host memory");
  }
}

int qp_nullifier_set_check(const uint64_t root[4], uint64_t m, const uint64_t x[4], uint32_t found, uint64_t pos,
                           const uint64_t lo_key[4], uint64_t lo_seq, const uint64_t *lo_siblings, uint32_t lo_bits,
                           uint32_t lo_depth, const uint64_t hi_key[4], uint64_t hi_seq, const uint64_t *hi_siblings,
                           uint32_t hi_bits, uint32_t hi_depth) {
  if (!root || !x || !lo_key || !lo_siblings || !hi_key || !hi_siblings) return QP_RECEIPT_NULL;
  return qns::check(root, m, x, found, pos, qns::Slot{lo_key, lo_seq, lo_siblings, lo_bits, lo_depth},
                    qns::Slot{hi_key, hi_seq, hi_siblings, hi_bits, hi_depth});
}

}  // extern "C"
