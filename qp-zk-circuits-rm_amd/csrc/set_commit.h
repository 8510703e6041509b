// set_commit.h — the owner of one nullifier-set commitment (set_root, m)
// beside the log's LogCommit (log_commit.h; nullifier_set.h has the
// definitions): the host path's sorted records and tree, or the device path's
// two record buffers and AccTree, with m, the root and the admitted count they
// were built at.  qp_ballot_box (ballot.cpp) and qp_ledger (ledger.cpp) each
// hold one, and qp_nullifier_set_root (nullifier_set.cpp) builds one for its
// call.  The set is rebuilt whole by a commit, because sorted positions move; a
// commit at the admitted count it was built at does nothing.  Its buffers are
// its own (sized for m, not for the handle's capacity), so a reserve does not
// touch it, and a handle that never asks for a set root allocates nothing.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../include/qpgpu.h"
#include "acc_tree.h"
#include "ledger_kernels.h"
#include "log_commit.h"
#include "nullifier_set.h"
#include "nullifier_set_kernels.h"

// the stage times of the last device build on this thread (SetCommit::times' layout), for qp_nullifier_set_times
inline std::vector<double> &set_commit_last_times() {
  thread_local std::vector<double> t;
  return t;
}

struct SetCommit {
  static constexpr uint64_t NEVER = ~0ull;
  // the stages a device commit times: select, tile sort, duplicates + leaves, levels, then the merge passes
  static constexpr uint32_t FIXED_STAGES = 4, MAX_STAGES = FIXED_STAGES + 32;
  // the events of a commit with np merge passes: 0 the start, 1 the select's end, 2 the tile sort's,
  // 3 + p merge pass p's, 3 + np the leaves', 4 + np the levels'

  qns::HostSet hset;           // the host path's
  AccTree tree;                // the device path's, laid out for m
  DevBuf d_key[2], d_seq[2];   // the two record buffers; `cur` holds the sorted set
  uint32_t cur = 0;
  uint64_t m = 0, built_at = NEVER;  // built_at: the admitted count of the log the set was made from
  uint64_t root[4] = {0, 0, 0, 0};
  uint64_t dup = qns::NOT_FOUND;  // the lowest duplicate member the last build found (a handle's log has none)
  DevBuf d_q, d_pos, d_found, d_gkey, d_gseq;  // per proofs batch (ACC_BATCH queries)
  TimingEvents<MAX_STAGES + 1> ev;
  bool timed = false;    // the last device commit built a set and recorded every event
  uint32_t npasses = 0;  // its merge passes

  qpk::NsetRecs recs(uint32_t i) const { return {d_key[i].p, d_seq[i].as<uint32_t>()}; }

  void drop() {
    hset.drop();
    tree.drop();
    for (int i = 0; i < 2; i++) d_key[i].release(), d_seq[i].release();
    m = 0;
    built_at = NEVER;
    dup = qns::NOT_FOUND;
    memset(root, 0, 32);
  }

  // (root, m) into a call's outputs, either of which may be null
  void pair(uint64_t root_out[4], uint64_t *m_out) const {
    if (root_out) memcpy(root_out, root, 32);
    if (m_out) *m_out = m;
  }

  // The host path: the set of log [0, n) (nullifiers [n][4], flags [n], the member bit `mask`).
  // *dup = NOT_FOUND or the lowest duplicate member; the set counts either way (the caller decides).
  void commit_host(const uint64_t *nullifiers, const uint8_t *flags, uint64_t n, uint8_t mask, uint64_t *dup) {
    if (built_at != n) {
      built_at = NEVER;
      hset.build(nullifiers, flags, n, mask);
      m = hset.m();
      memcpy(root, hset.root, 32);
      built_at = n;
      this->dup = hset.dup;
    }
    *dup = this->dup;
  }

  int stamp(AccErr e, hipStream_t s, uint32_t i) {
    if (!ev.e[i]) QP_HIP_TRY(&e, hipEventCreate(&ev.e[i]));
    QP_HIP_TRY(&e, hipEventRecord(ev.e[i], s));
    return QP_OK;
  }

  // The device path: the set of log [0, n), n <= 2^31 (nullifier [n][4] and flags [n] on the device,
  // final on c's stream).  Select, one synchronise for m, tile sort, merge passes, duplicates, leaves,
  // levels, one synchronise for the root and the duplicate word.  *dup as above.  A failed step
  // leaves no set (built_at = NEVER).
  int commit_device(qp_ctx *c, std::string &err, const uint64_t *nullifier, const uint8_t *flags, uint64_t n, uint8_t mask,
                    uint64_t *dup) {
    *dup = this->dup;
    if (built_at == n) return QP_OK;
    built_at = NEVER;
    *dup = this->dup = qns::NOT_FOUND;
    timed = false;
    hipStream_t s = c->stream;
    AccErr e{err};
    QP_HIP_TRY(&e, hipSetDevice(c->device));
    tree.drop();
    m = 0;
    memset(root, 0, 32);
    if (!n) {
      built_at = 0;
      return QP_OK;
    }
    const uint32_t nb = qpk::ledger_blocks(n);
    DevBuf d_blk, d_sel;  // the call's own: block counts (+ total, + the duplicate word), the members in log order
    QP_HIP_TRY(&e, d_blk.alloc(((size_t)nb + 3) / 2));
    QP_HIP_TRY(&e, d_sel.alloc((n + 1) / 2));
    uint32_t *blk = d_blk.as<uint32_t>(), *sel = d_sel.as<uint32_t>(), *d_dup = blk + nb + 1;
    uint32_t total = 0, word = qpk::NSET_NO_SEQ;
    if (int rc = stamp(e, s, 0)) return rc;
    qpk::nset_select_count(flags, (uint32_t)n, mask, blk, s);
    QP_HIP_TRY(&e, hipGetLastError());
    qpk::ledger_scan(blk, nb, blk + nb, s);
    QP_HIP_TRY(&e, hipGetLastError());
    qpk::nset_select_write(flags, (uint32_t)n, mask, blk, sel, s);
    QP_HIP_TRY(&e, hipGetLastError());
    QP_HIP_TRY(&e, hipMemcpyAsync(&total, blk + nb, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipMemcpyAsync(d_dup, &word, 4, hipMemcpyHostToDevice, s));
    if (int rc = stamp(e, s, 1)) return rc;
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    if (total > n) {
      err = "the set's select counted more members than the log has entries (an internal invariant broke)";
      return QP_ERR_HIP;
    }
    if (!total) {
      built_at = n;
      return QP_OK;
    }
    for (int i = 0; i < 2; i++)
      if (d_seq[i].words * 2 < total || d_seq[i].words > (size_t)total) {  // too small, or more than twice what is needed
        QP_HIP_TRY(&e, d_key[i].alloc((size_t)total * 4));
        QP_HIP_TRY(&e, d_seq[i].alloc(((size_t)total + 1) / 2));
      }
    qpk::nset_tile_sort(nullifier, sel, total, recs(0), s);
    QP_HIP_TRY(&e, hipGetLastError());
    if (int rc = stamp(e, s, 2)) return rc;
    uint32_t at = 0, npass = 0;
    for (uint64_t run = qpk::NSET_TILE; run < total; run *= 2, at ^= 1, npass++) {
      qpk::nset_merge(recs(at), recs(at ^ 1), total, (uint32_t)run, s);
      QP_HIP_TRY(&e, hipGetLastError());
      if (int rc = stamp(e, s, 3 + npass)) return rc;
    }
    qpk::nset_duplicates(recs(at), total, d_dup, s);
    QP_HIP_TRY(&e, hipGetLastError());
    const qpk::NsetRecs sorted = recs(at);
    auto leaves = [&](uint32_t, uint32_t end, uint64_t *dig) { qpk::nset_leaves(sorted, end, dig, s); };
    qpk::AccLevels lv;
    uint64_t now[4];
    // log_tree_whole's steps, with a stamp between the leaves and the levels
    if (int rc = tree.alloc(e, total)) return rc;
    qpk::acc_levels_reserved(total, total, lv);
    leaves(0, total, tree.dig.p);
    QP_HIP_TRY(&e, hipGetLastError());
    if (int rc = stamp(e, s, 3 + npass)) return rc;
    tree.append(lv, qpk::acc_row_max(), s);
    QP_HIP_TRY(&e, hipGetLastError());
    QP_HIP_TRY(&e, hipMemcpyAsync(now, tree.root(lv), 32, hipMemcpyDeviceToHost, s));
    if (int rc = stamp(e, s, 4 + npass)) return rc;
    QP_HIP_TRY(&e, hipMemcpyAsync(&word, d_dup, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    tree.lv = lv;
    cur = at;
    m = total;
    memcpy(root, now, 32);
    npasses = npass;
    timed = true;
    built_at = n;
    std::vector<double> &t = set_commit_last_times();
    t.resize(FIXED_STAGES + npass);
    times(t.data(), (uint32_t)t.size());
    if (word != qpk::NSET_NO_SEQ) *dup = this->dup = word;
    return QP_OK;
  }

  // The stage times of the last device commit that built a set (ms): out[0..4) = select, tile sort,
  // duplicates + leaves, levels; out[4 + p] = merge pass p.  Returns the number written (0: none).
  // The tile sort's span includes the host's wait for m.
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

  int query_buffers(AccErr e) {
    if (d_q.p) return QP_OK;
    QP_HIP_TRY(&e, d_pos.alloc(ACC_BATCH / 2));
    QP_HIP_TRY(&e, d_found.alloc(ACC_BATCH / 2));
    QP_HIP_TRY(&e, d_gkey.alloc((size_t)ACC_BATCH * 4));
    QP_HIP_TRY(&e, d_gseq.alloc(ACC_BATCH));
    QP_HIP_TRY(&e, d_q.alloc((size_t)ACC_BATCH * 4));
    return QP_OK;
  }

  // After a commit: the proofs of keys[k][4] (canonical; the caller checked) under (root, m), laid
  // out as qp_*_set_proofs documents: found [k], pos [k]; per slot key [k][4], seq [k], siblings
  // [k][32][4], bits [k], depth [k]; a slot the proof has no use for is all zero.  c null: the host path.
  struct Out {
    uint8_t *found;
    uint64_t *pos;
    uint64_t *key[2], *seq[2], *sib[2];  // 0: lo, 1: hi
    uint32_t *bits[2], *depth[2];
  };
  int proofs(qp_ctx *c, std::string &err, const uint64_t *keys, uint32_t k, const Out &o) {
    for (int sl = 0; sl < 2; sl++) {
      memset(o.key[sl], 0, (size_t)k * 32);
      memset(o.seq[sl], 0, (size_t)k * 8);
      memset(o.sib[sl], 0, (size_t)k * qpk::ACC_PATH_SLOTS * 32);
      memset(o.bits[sl], 0, (size_t)k * 4);
      memset(o.depth[sl], 0, (size_t)k * 4);
    }
    if (!c) {
      for (uint32_t i = 0; i < k; i++) {
        bool f;
        const uint64_t p = hset.search(keys + (size_t)i * 4, &f);
        o.found[i] = f;
        o.pos[i] = p;
        const bool has[2] = {!f && p > 0, p < m};
        const uint64_t at[2] = {p - 1, p};
        for (int sl = 0; sl < 2; sl++) {
          if (!has[sl]) continue;
          memcpy(o.key[sl] + (size_t)i * 4, &hset.keys[at[sl] * 4], 32);
          o.seq[sl][i] = hset.seqs[at[sl]];
          hset.tree.path(at[sl], o.sib[sl] + (size_t)i * qpk::ACC_PATH_SLOTS * 4, o.bits[sl] + i, o.depth[sl] + i, nullptr);
        }
      }
      return QP_OK;
    }
    hipStream_t s = c->stream;
    AccErr e{err};
    QP_HIP_TRY(&e, hipSetDevice(c->device));
    if (!m) {  // every absence holds with no path
      memset(o.found, 0, k);
      memset(o.pos, 0, (size_t)k * 8);
      return QP_OK;
    }
    if (int rc = query_buffers(e)) return rc;
    const qpk::NsetRecs sorted = recs(cur);
    std::vector<uint32_t> hp(std::min(k, ACC_BATCH)), hf(hp.size());
    std::vector<uint64_t> idx, gkey, gseq, sib;
    std::vector<uint32_t> bits, depth, where;  // where[j] = query << 1 | slot of gathered position j
    for (uint32_t done = 0; done < k;) {
      const uint32_t nb = std::min(ACC_BATCH, k - done);
      QP_HIP_TRY(&e, hipMemcpyAsync(d_q.p, keys + (size_t)done * 4, (size_t)nb * 32, hipMemcpyHostToDevice, s));
      qpk::nset_search(sorted, (uint32_t)m, d_q.p, nb, d_pos.as<uint32_t>(), d_found.as<uint32_t>(), s);
      QP_HIP_TRY(&e, hipGetLastError());
      QP_HIP_TRY(&e, hipMemcpyAsync(hp.data(), d_pos.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
      QP_HIP_TRY(&e, hipMemcpyAsync(hf.data(), d_found.p, (size_t)nb * 4, hipMemcpyDeviceToHost, s));
      QP_HIP_TRY(&e, hipStreamSynchronize(s));
      idx.clear();
      where.clear();
      for (uint32_t i = 0; i < nb; i++) {
        const uint64_t p = hp[i];
        if (p > m) {
          err = "the set's search answered a position beyond the set (an internal invariant broke)";
          return QP_ERR_HIP;
        }
        o.found[done + i] = hf[i] != 0;
        o.pos[done + i] = p;
        if (!hf[i] && p > 0) idx.push_back(p - 1), where.push_back((done + i) << 1);
        if (p < m) idx.push_back(p), where.push_back((done + i) << 1 | 1);
      }
      // at most 2 nb positions: in pieces of ACC_BATCH, the size of the gather's and the paths' buffers
      const size_t cnt = idx.size();
      gkey.resize(cnt * 4), gseq.resize(cnt), sib.resize(cnt * qpk::ACC_PATH_SLOTS * 4), bits.resize(cnt), depth.resize(cnt);
      for (size_t g = 0; g < cnt; g += ACC_BATCH) {
        const uint32_t ng = (uint32_t)std::min<size_t>(ACC_BATCH, cnt - g);
        QP_HIP_TRY(&e, hipMemcpyAsync(d_q.p, idx.data() + g, (size_t)ng * 8, hipMemcpyHostToDevice, s));
        qpk::nset_gather(sorted, d_q.p, ng, d_gkey.p, d_gseq.p, s);
        QP_HIP_TRY(&e, hipGetLastError());
        QP_HIP_TRY(&e, hipMemcpyAsync(gkey.data() + g * 4, d_gkey.p, (size_t)ng * 32, hipMemcpyDeviceToHost, s));
        QP_HIP_TRY(&e, hipMemcpyAsync(gseq.data() + g, d_gseq.p, (size_t)ng * 8, hipMemcpyDeviceToHost, s));
        QP_HIP_TRY(&e, hipStreamSynchronize(s));
      }
      if (cnt)
        if (int rc = tree.paths(e, s, idx.data(), (uint32_t)cnt, sib.data(), bits.data(), depth.data(), nullptr)) return rc;
      for (size_t j = 0; j < cnt; j++) {
        const uint32_t i = where[j] >> 1, sl = where[j] & 1;
        memcpy(o.key[sl] + (size_t)i * 4, &gkey[j * 4], 32);
        o.seq[sl][i] = gseq[j];
        memcpy(o.sib[sl] + (size_t)i * qpk::ACC_PATH_SLOTS * 4, &sib[j * qpk::ACC_PATH_SLOTS * 4], qpk::ACC_PATH_SLOTS * 32);
        o.bits[sl][i] = bits[j];
        o.depth[sl][i] = depth[j];
      }
      done += nb;
    }
    return QP_OK;
  }
};
