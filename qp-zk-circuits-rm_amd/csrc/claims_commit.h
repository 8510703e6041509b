// claims_commit.h — the owner of one payout claims commitment (claims_root, A,
// total) beside the ledger's LogCommit and SetCommit (set_commit.h; claims.h has
// the definitions): the host path's sorted rows and tree, or the device path's
// two record buffers, per-position totals and an AccTree laid out for A.
// qp_ledger (ledger.cpp) holds one, and qp_ledger_log_claims_root (claims.cpp)
// builds one for its call.  It is keyed by the range (m0, m1): the log is
// append-only and final, so a range's commitment never changes; the same range
// again launches nothing, another range rebuilds.  Its buffers are its own
// (sized for A), so a reserve does not touch it, and a ledger that never asks
// for a claims root allocates nothing.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/qpgpu.h"
#include "acc_tree.h"
#include "claims.h"
#include "claims_kernels.h"
#include "ledger_audit_device.h"
#include "ledger_kernels.h"
#include "ledger_rounds.h"
#include "nullifier_set_kernels.h"

// the stage times of the last device build on this thread (ClaimsCommit::times' layout), for qp_ledger_claims_times
inline std::vector<double> &claims_commit_last_times() {
  thread_local std::vector<double> t;
  return t;
}

struct ClaimsCommit {
  // the stages a device build times: credit + compaction, tile sort, leaves + total, levels, then the merge passes
  static constexpr uint32_t FIXED_STAGES = 4, MAX_STAGES = FIXED_STAGES + 32;
  // the events of a build with np merge passes: 0 the start, 1 the credit's end (after the host's wait
  // for A), 2 the tile sort's, 3 + p merge pass p's, 3 + np the leaves' and the total's, 4 + np the levels'

  qcl::HostClaims host;       // the host path's
  AccTree tree;               // the device path's, laid out for A
  DevBuf d_key[2], d_seq[2];  // the two record buffers (account, local entry index); `cur` holds the sorted rows
  DevBuf d_tot;               // totals [A][5] by sorted position
  uint32_t cur = 0;
  bool built = false;  // (m0, m1) names the range the members below belong to
  uint64_t m0 = 0, m1 = 0, A = 0;
  uint64_t root[4] = {0, 0, 0, 0};
  uint32_t total[5] = {0, 0, 0, 0, 0};
  DevBuf d_q, d_pos, d_found, d_gkey, d_gseq, d_gtot;  // per proofs batch (ACC_BATCH queries)
  TimingEvents<MAX_STAGES + 1> ev;
  bool timed = false;
  uint32_t npasses = 0;

  qpk::NsetRecs recs(uint32_t i) const { return {d_key[i].p, d_seq[i].as<uint32_t>()}; }

  void drop() {
    host.drop();
    tree.drop();
    for (int i = 0; i < 2; i++) d_key[i].release(), d_seq[i].release();
    d_tot.release();
    built = false;
    A = 0;
    memset(root, 0, 32);
    memset(total, 0, sizeof total);
  }

  bool has(uint64_t a, uint64_t b) const { return built && m0 == a && m1 == b; }

  // (root, A, total) into a call's outputs, each of which may be null
  void triple(uint64_t root_out[4], uint64_t *count_out, uint32_t total_out[5]) const {
    if (root_out) memcpy(root_out, root, 32);
    if (count_out) *count_out = A;
    if (total_out) memcpy(total_out, total, sizeof total);
  }

  // The host path: range [a, b) of a log in qp_ledger_entries' layout (indexed by seq from 0).
  void commit_host(const uint64_t *accounts_log, const uint32_t *amounts, const uint8_t *flags, uint64_t a, uint64_t b) {
    if (has(a, b)) return;
    drop();
    ql::RoundRows rows;
    ql::round_payouts_host(accounts_log, amounts, flags, a, b, rows);
    host.build(rows);
    A = host.count();
    memcpy(root, host.root, 32);
    memcpy(total, host.total, sizeof total);
    m0 = a, m1 = b;
    built = true;
  }

  int stamp(AccErr e, hipStream_t s, uint32_t i) {
    if (!ev.e[i]) QP_HIP_TRY(&e, hipEventCreate(&ev.e[i]));
    QP_HIP_TRY(&e, hipEventRecord(ev.e[i], s));
    return QP_OK;
  }

  // The device path: range [a, b), b - a <= 2^31; the pointers are device pointers at entry a of a
  // log that is final on c's stream.  The payout round's credit and compaction (one synchronise for
  // A), the nullifier set's tile sort and merge passes over (account column, owners), the leaves,
  // the grand total, the levels, one synchronise for the root, the total and the error word.  A
  // failed step leaves no commitment.
  int commit_device(qp_ctx *c, std::string &err, const uint64_t *accounts_at, const uint32_t *amounts_at,
                    const uint8_t *flags_at, uint64_t a, uint64_t b) {
    if (has(a, b)) return QP_OK;
    drop();
    timed = false;
    hipStream_t s = c->stream;
    AccErr e{err};
    QP_HIP_TRY(&e, hipSetDevice(c->device));
    const uint64_t k = b - a;
    if (!k) {
      m0 = a, m1 = b, built = true;
      return QP_OK;
    }
    qla::RoundCredit r;  // the call's own scratch, freed when it returns
    if (int rc = stamp(e, s, 0)) return rc;
    if (int rc = qla::round_credit_device(c, err, accounts_at, amounts_at, flags_at, k, r)) return rc;
    if (int rc = stamp(e, s, 1)) return rc;
    const uint32_t rows = r.rows;
    if (!rows) {
      m0 = a, m1 = b, built = true;
      return QP_OK;
    }
    for (int i = 0; i < 2; i++) {
      QP_HIP_TRY(&e, d_key[i].alloc((size_t)rows * 4));
      QP_HIP_TRY(&e, d_seq[i].alloc(((size_t)rows + 1) / 2));
    }
    QP_HIP_TRY(&e, d_tot.alloc(((size_t)rows * qcl::LIMBS + 1) / 2));
    DevBuf d_sum;  // the four limb sums of the grand total, then the error word
    QP_HIP_TRY(&e, d_sum.alloc(5));
    QP_HIP_TRY(&e, hipMemsetAsync(d_sum.p, 0, 40, s));
    unsigned long long *gsum = d_sum.as<unsigned long long>();
    uint32_t *d_err = reinterpret_cast<uint32_t *>(d_sum.p + 4);
    qpk::nset_tile_sort(r.v.account, r.payee(), rows, recs(0), s);
    QP_HIP_TRY(&e, hipGetLastError());
    if (int rc = stamp(e, s, 2)) return rc;
    uint32_t at = 0, npass = 0;
    for (uint64_t run = qpk::NSET_TILE; run < rows; run *= 2, at ^= 1, npass++) {
      qpk::nset_merge(recs(at), recs(at ^ 1), rows, (uint32_t)run, s);
      QP_HIP_TRY(&e, hipGetLastError());
      if (int rc = stamp(e, s, 3 + npass)) return rc;
    }
    const qpk::NsetRecs sorted = recs(at);
    qpk::AccLevels lv;
    uint64_t now[4], sums[4];
    uint32_t word = 0;
    if (int rc = tree.alloc(e, rows)) return rc;
    qpk::acc_levels_reserved(rows, rows, lv);
    qpk::claims_leaves(sorted, rows, r.v, (uint32_t)k, a, d_tot.as<uint32_t>(), tree.dig.p, d_err, s);
    QP_HIP_TRY(&e, hipGetLastError());
    qpk::claims_total(sorted.seq, rows, r.v, (uint32_t)k, gsum, d_err, s);
    QP_HIP_TRY(&e, hipGetLastError());
    if (int rc = stamp(e, s, 3 + npass)) return rc;
    tree.append(lv, qpk::acc_row_max(), s);
    QP_HIP_TRY(&e, hipGetLastError());
    QP_HIP_TRY(&e, hipMemcpyAsync(now, tree.root(lv), 32, hipMemcpyDeviceToHost, s));
    if (int rc = stamp(e, s, 4 + npass)) return rc;
    QP_HIP_TRY(&e, hipMemcpyAsync(sums, gsum, 32, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(&word, d_err, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    if (word) {
      tree.drop();
      err = std::string(word & qpk::CLAIMS_ERR_ENTRY ? "a claims record names an entry outside the range"
                                                      : "a claims record's entry has no account slot") +
            " (an internal invariant broke)";
      return QP_ERR_HIP;
    }
    tree.lv = lv;
    cur = at;
    A = rows;
    memcpy(root, now, 32);
    qcl::normalise(sums, total);
    npasses = npass;
    timed = true;
    m0 = a, m1 = b, built = true;
    std::vector<double> &t = claims_commit_last_times();
    t.resize(FIXED_STAGES + npass);
    times(t.data(), (uint32_t)t.size());
    return QP_OK;
  }

  // The stage times of the last device build that made a tree (ms): out[0..4) = credit + compaction
  // (with the scratch's allocation and the host's wait for A), tile sort, leaves + total, levels;
  // out[4 + p] = merge pass p.  Returns the number written (0: none).
  uint32_t times(double *out, uint32_t cap) {
    if (!timed || cap < FIXED_STAGES + npasses) return 0;
    auto span = [&](uint32_t a, uint32_t b) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, ev.e[a], ev.e[b]);
      return (double)ms;
    };
    out[0] = span(0, 1);
    out[1] = span(1, 2);
    out[2] = span(2 + npasses, 3 + npasses);
    out[3] = span(3 + npasses, 4 + npasses);
    for (uint32_t p = 0; p < npasses; p++) out[FIXED_STAGES + p] = span(2 + p, 3 + p);
    return FIXED_STAGES + npasses;
  }

  // After a device commit: first_seq of the rows in sorted order into out[A] (host)
  int order_device(qp_ctx *c, std::string &err, uint64_t *out) {
    if (!A) return QP_OK;
    AccErr e{err};
    std::vector<uint32_t> h(A);
    QP_HIP_TRY(&e, hipSetDevice(c->device));
    QP_HIP_TRY(&e, hipMemcpyAsync(h.data(), recs(cur).seq, A * 4, hipMemcpyDeviceToHost, c->stream));
    QP_HIP_TRY(&e, hipStreamSynchronize(c->stream));
    for (uint64_t j = 0; j < A; j++) out[j] = m0 + h[j];
    return QP_OK;
  }

  int query_buffers(AccErr e) {
    if (d_q.p) return QP_OK;
    QP_HIP_TRY(&e, d_pos.alloc(ACC_BATCH / 2));
    QP_HIP_TRY(&e, d_found.alloc(ACC_BATCH / 2));
    QP_HIP_TRY(&e, d_gkey.alloc((size_t)ACC_BATCH * 4));
    QP_HIP_TRY(&e, d_gseq.alloc(ACC_BATCH));
    QP_HIP_TRY(&e, d_gtot.alloc(((size_t)ACC_BATCH * qcl::LIMBS + 1) / 2));
    QP_HIP_TRY(&e, d_q.alloc((size_t)ACC_BATCH * 4));
    return QP_OK;
  }

  // After a commit: the claims of accounts keys[k][4] (canonical; the caller checked) under (root,
  // A), laid out as qp_ledger_claims documents: found [k], pos [k]; per slot account [k][4], total
  // [k][5], first_seq [k], siblings [k][32][4], bits [k], depth [k]; a slot the claim has no use for
  // is all zero.  c null: the host path.
  struct Out {
    uint8_t *found;
    uint64_t *pos;
    uint64_t *account[2];  // 0: lo, 1: hi
    uint32_t *total[2];
    uint64_t *first_seq[2], *sib[2];
    uint32_t *bits[2], *depth[2];
  };
  int proofs(qp_ctx *c, std::string &err, const uint64_t *keys, uint32_t k, const Out &o) {
    for (int sl = 0; sl < 2; sl++) {
      memset(o.account[sl], 0, (size_t)k * 32);
      memset(o.total[sl], 0, (size_t)k * qcl::LIMBS * 4);
      memset(o.first_seq[sl], 0, (size_t)k * 8);
      memset(o.sib[sl], 0, (size_t)k * qpk::ACC_PATH_SLOTS * 32);
      memset(o.bits[sl], 0, (size_t)k * 4);
      memset(o.depth[sl], 0, (size_t)k * 4);
    }
    if (!A) {  // every absence holds with no path
      memset(o.found, 0, k);
      memset(o.pos, 0, (size_t)k * 8);
      return QP_OK;
    }
    if (!c) {
      for (uint32_t i = 0; i < k; i++) {
        bool f;
        const uint64_t p = host.search(keys + (size_t)i * 4, &f);
        o.found[i] = f;
        o.pos[i] = p;
        const bool has[2] = {!f && p > 0, p < A};
        const uint64_t at[2] = {p - 1, p};
        for (int sl = 0; sl < 2; sl++) {
          if (!has[sl]) continue;
          memcpy(o.account[sl] + (size_t)i * 4, &host.accounts[at[sl] * 4], 32);
          memcpy(o.total[sl] + (size_t)i * qcl::LIMBS, &host.totals[at[sl] * qcl::LIMBS], qcl::LIMBS * 4);
          o.first_seq[sl][i] = host.first_seq[at[sl]];
          host.tree.path(at[sl], o.sib[sl] + (size_t)i * qpk::ACC_PATH_SLOTS * 4, o.bits[sl] + i, o.depth[sl] + i, nullptr);
        }
      }
      return QP_OK;
    }
    hipStream_t s = c->stream;
    AccErr e{err};
    QP_HIP_TRY(&e, hipSetDevice(c->device));
    if (int rc = query_buffers(e)) return rc;
    const qpk::NsetRecs sorted = recs(cur);
    std::vector<uint32_t> hp(std::min(k, ACC_BATCH)), hf(hp.size());
    std::vector<uint64_t> idx, gkey, gseq, sib;
    std::vector<uint32_t> gtot, bits, depth, where;  // where[j] = query << 1 | slot of gathered position j
    for (uint32_t done = 0; done < k;) {
      const uint32_t nb = std::min(ACC_BATCH, k - done);
      QP_HIP_TRY(&e, hipMemcpyAsync(d_q.p, keys + (size_t)done * 4, (size_t)nb * 32, hipMemcpyHostToDevice, s));
      qpk::nset_search(sorted, (uint32_t)A, d_q.p, nb, d_pos.as<uint32_t>(), d_found.as<uint32_t>(), s);
      QP_HIP_TRY(&e, hipGetLastError());
      QP_HIP_TRY(&e, hipMemcpyAsync(hp.data(), d_pos.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
      QP_HIP_TRY(&e, hipMemcpyAsync(hf.data(), d_found.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
      QP_HIP_TRY(&e, hipStreamSynchronize(s));
      idx.clear();
      where.clear();
      for (uint32_t i = 0; i < nb; i++) {
        const uint64_t p = hp[i];
        if (p > A) {
          err = "the claims' search answered a position beyond the rows (an internal invariant broke)";
          return QP_ERR_HIP;
        }
        o.found[done + i] = hf[i] != 0;
        o.pos[done + i] = p;
        if (!hf[i] && p > 0) idx.push_back(p - 1), where.push_back((done + i) << 1);
        if (p < A) idx.push_back(p), where.push_back((done + i) << 1 | 1);
      }
      // at most 2 nb positions, each below A: in pieces of ACC_BATCH, the size of the gathers' and the paths' buffers
      const size_t cnt = idx.size();
      gkey.resize(cnt * 4), gseq.resize(cnt), gtot.resize(cnt * qcl::LIMBS);
      sib.resize(cnt * qpk::ACC_PATH_SLOTS * 4), bits.resize(cnt), depth.resize(cnt);
      for (size_t g = 0; g < cnt; g += ACC_BATCH) {
        const uint32_t ng = (uint32_t)std::min<size_t>(ACC_BATCH, cnt - g);
        QP_HIP_TRY(&e, hipMemcpyAsync(d_q.p, idx.data() + g, (size_t)ng * 8, hipMemcpyHostToDevice, s));
        qpk::nset_gather(sorted, d_q.p, ng, d_gkey.p, d_gseq.p, s);
        QP_HIP_TRY(&e, hipGetLastError());
        qpk::claims_gather_totals(d_tot.as<uint32_t>(), d_q.p, ng, d_gtot.as<uint32_t>(), s);
        QP_HIP_TRY(&e, hipGetLastError());
        QP_HIP_TRY(&e, hipMemcpyAsync(gkey.data() + g * 4, d_gkey.p, (size_t)ng * 32, hipMemcpyDeviceToHost, s));
        QP_HIP_TRY(&e, hipMemcpyAsync(gseq.data() + g, d_gseq.p, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
        QP_HIP_TRY(&e, hipMemcpyAsync(gtot.data() + g * qcl::LIMBS, d_gtot.p, (size_t)ng * qcl::LIMBS * 4,
                                      hipMemcpyDeviceToHost, s));
        QP_HIP_TRY(&e, hipStreamSynchronize(s));
      }
      if (cnt)
        if (int rc = tree.paths(e, s, idx.data(), (uint32_t)cnt, sib.data(), bits.data(), depth.data(), nullptr)) return rc;
      for (size_t j = 0; j < cnt; j++) {
        const uint32_t i = where[j] >> 1, sl = where[j] & 1;
        memcpy(o.account[sl] + (size_t)i * 4, &gkey[j * 4], 32);
        memcpy(o.total[sl] + (size_t)i * qcl::LIMBS, &gtot[j * qcl::LIMBS], qcl::LIMBS * 4);
        o.first_seq[sl][i] = m0 + gseq[j];  // a record holds the entry's index within the range
        memcpy(o.sib[sl] + (size_t)i * qpk::ACC_PATH_SLOTS * 4, &sib[j * qpk::ACC_PATH_SLOTS * 4], qpk::ACC_PATH_SLOTS * 32);
        o.bits[sl][i] = bits[j];
        o.depth[sl][i] = depth[j];
      }
      done += nb;
    }
    return QP_OK;
  }
};
