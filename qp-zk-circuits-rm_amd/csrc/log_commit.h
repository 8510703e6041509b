// log_commit.h — the owner of one log commitment (root, n): the host path's
// tree, the device path's AccTree, the leaves committed so far and the root
// over them.  qp_ballot_box (ballot.cpp) and qp_ledger (ledger.cpp) each hold
// one.  The tree is built by the first commit, laid out for the handle's
// capacity, and dropped by a reserve; a cast does not touch it.  The leaf
// kernel, the defensive error word's text and the return code of a broken
// invariant stay with the handle.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include "../../include/qpgpu.h"
#include "acc_tree.h"

// Enqueues on s what brings `tree` from its n() leaves to table lv (of the tree's layout): the
// handle's leaf kernel, leaves(first, end, dig) for [n(), lv.len[0]), the levels above them, and the
// copy of the new root into root (host).  The caller synchronises and only then sets tree.lv = lv.
template <class Leaves>
int log_tree_append(AccErr e, hipStream_t s, const AccTree &tree, const qpk::AccLevels &lv, Leaves leaves, uint64_t root[4]) {
  leaves((uint32_t)tree.n(), (uint32_t)lv.len[0], tree.dig.p);
  QP_HIP_TRY(&e, hipGetLastError());
  tree.append(lv, qpk::acc_row_max(), s);
  QP_HIP_TRY(&e, hipGetLastError());
  QP_HIP_TRY(&e, hipMemcpyAsync(root, tree.root(lv), 32, hipMemcpyDeviceToHost, s));
  return QP_OK;
}

// The whole log into an empty tree of n leaves, 1 <= n <= 2^31 (an audit's tree: the caller checked
// n): allocates `tree` (an AccTree without a tree) for n and enqueues every level; lv and root as above.
template <class Leaves>
int log_tree_whole(AccErr e, hipStream_t s, AccTree &tree, uint64_t n, Leaves leaves, qpk::AccLevels &lv, uint64_t root[4]) {
  if (int rc = tree.alloc(e, n)) return rc;
  qpk::acc_levels_reserved(n, n, lv);
  return log_tree_append(e, s, tree, lv, leaves, root);
}

template <class HostLog>
struct LogCommit {
  HostLog hlog;            // the host path's tree
  AccTree log;             // the device path's, laid out for the handle's capacity
  uint64_t committed = 0;  // leaves of the tree = the n of (root, n)
  uint64_t root[4] = {0, 0, 0, 0};

  // the tree's layout is the capacity's: a reserve drops it, and the next commit rebuilds it from
  // the log, which gives the same root
  void drop() {
    hlog.drop();
    log.drop();
    committed = 0;
  }

  // The host path: the tree up to host's log.  false: HostLog::commit refused (a number >= p).
  template <class Host>
  bool commit(const Host &host) {
    if (!hlog.commit(host)) return false;
    memcpy(root, hlog.root(), 32);
    committed = hlog.n;
    return true;
  }

  // The device path: the tree up to `count` > 0 leaves of a log with room for `capacity`.  Nothing is
  // done when `count` are committed.  Else leaves [committed, count) through leaves(first, end, dig),
  // the levels above them, the root and the handle's error word (device, d_word) in one synchronise.
  // *word != 0: the handle translates it, and nothing of this commit counts.  `broken`: the handle's
  // return code for a log that does not fit its capacity (fn names the call in that text).
  template <class Leaves>
  int commit(qp_ctx *c, std::string &err, const char *fn, int broken, uint64_t count, uint64_t capacity, Leaves leaves,
             const uint32_t *d_word, uint32_t *word) {
    *word = 0;
    if (committed == count) return QP_OK;
    hipStream_t s = c->stream;
    AccErr e{err};
    QP_HIP_TRY(&e, hipSetDevice(c->device));
    if (!log.dig.p)
      if (int rc = log.alloc(e, capacity)) return rc;
    qpk::AccLevels lv;
    if (!qpk::acc_levels_reserved(count, capacity, lv)) {
      err = std::string(fn) + ": the log does not fit its capacity (an internal invariant broke)";
      return broken;
    }
    uint64_t now[4];
    if (int rc = log_tree_append(e, s, log, lv, leaves, now)) return rc;  // the tree holds `committed` leaves
    QP_HIP_TRY(&e, hipMemcpyAsync(word, d_word, 4, hipMemcpyDeviceToHost, s));
    QP_HIP_TRY(&e, hipStreamSynchronize(s));
    if (*word) return QP_OK;
    memcpy(root, now, 32);
    log.lv = lv;
    committed = count;
    return QP_OK;
  }

  // (root, n) into a call's outputs, either of which may be null
  void pair(uint64_t root_out[4], uint64_t *n_out) const {
    if (root_out) memcpy(root_out, root, 32);
    if (n_out) *n_out = committed;
  }

  // The tail of *_receipts after a commit: the paths of seqs[k], each < committed (the caller checked),
  // laid out as k_acc_paths writes them; leaves may be null.  c null: the host path.
  int receipts(qp_ctx *c, std::string &err, const uint64_t *seqs, uint32_t k, uint64_t *siblings, uint32_t *path_bits,
               uint32_t *depth, uint64_t *leaves) {
    if (c) {
      AccErr e{err};
      QP_HIP_TRY(&e, hipSetDevice(c->device));
      return log.paths(e, c->stream, seqs, k, siblings, path_bits, depth, leaves);
    }
    for (uint32_t i = 0; i < k; i++)
      hlog.path(seqs[i], siblings + (size_t)i * qpk::ACC_PATH_SLOTS * 4, path_bits + i, depth + i,
                leaves ? leaves + (size_t)i * 4 : nullptr);
    return QP_OK;
  }

  // The tail of *_roots_at after a commit: roots_out[i][4] = the root the log had at ms[i] leaves, each
  // in 1..committed (the caller checked).  node: the log's node hash, for the host path.
  template <class NodeHash>
  int roots_at(qp_ctx *c, std::string &err, const uint64_t *ms, uint32_t k, NodeHash node, uint64_t *roots_out) {
    if (c) {
      AccErr e{err};
      QP_HIP_TRY(&e, hipSetDevice(c->device));
      return log.prefix_roots(e, c->stream, ms, k, roots_out);
    }
    for (uint32_t i = 0; i < k; i++) hlog.prefix_root(ms[i], node, roots_out + (size_t)i * 4);
    return QP_OK;
  }
};
