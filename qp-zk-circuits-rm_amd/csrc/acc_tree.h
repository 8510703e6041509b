// acc_tree.h — the device owner of one accumulator tree (acc_kernels.h): the
// digest buffer, the level table and one batch of path buffers.  qp_registry
// holds one; qp_ballot_box and qp_ledger hold theirs in a LogCommit
// (log_commit.h), and each log audit builds one for its call.  The leaves,
// hipSetDevice, timing events and the moment a new size counts stay with the
// owner: the launching calls only launch, and the owner sets `lv` once its own
// synchronise succeeded.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>
#include "acc_kernels.h"
#include "ctx.h"

// where a call reports a failed HIP call: the err string of the handle that owns the tree
struct AccErr {
  std::string &err;
};

// leaves per k_acc_paths launch (the batch buffers hold this many paths: 8 MB of siblings)
constexpr uint32_t ACC_BATCH = 8192;

struct AccTree {
  DevBuf dig;             // [level][node][4]: acc_reserved(capacity) digests; dig.p is level 0
  qpk::AccLevels lv;      // the table of the current leaves in that layout
  uint64_t capacity = 0;  // 0: no tree (dig.p is null)
  DevBuf d_idx, d_sib, d_bits, d_depth, d_leaf;  // one batch of paths, allocated by the first
  DevBuf d_m, d_roots;                           // one batch of prefix-root queries, allocated by the first

  uint64_t n() const { return lv.nlevels ? lv.len[0] : 0; }
  // the root of the tree at table `at` (device)
  const uint64_t *root(const qpk::AccLevels &at) const { return dig.p + at.off[at.nlevels - 1] * 4; }
  // an empty tree (n() = 0) for `cap` leaves, 1 <= cap <= 2^31 (the caller checks)
  int alloc(AccErr e, uint64_t cap);
  // no tree; the path buffers stay
  void drop() {
    dig.release();
    lv = qpk::AccLevels();
    capacity = 0;
  }
  // launches the levels above level 0 for table nlv, after the caller wrote leaves [n(), nlv.len[0])
  void append(const qpk::AccLevels &nlv, uint64_t row_max, hipStream_t s) const {
    qpk::acc_append(dig.p, nlv, n(), row_max, s);
  }
  // launches qpk::acc_replace on the current table
  void replace(const uint64_t *idx, const uint64_t *leaves, uint32_t k, uint64_t row_max, hipStream_t s) const {
    qpk::acc_replace(dig.p, lv, idx, leaves, k, row_max, s);
  }
  // the paths (and, leaves != null, the leaf digests [nidx][4]) of leaves idx[] < n() (host; the caller
  // checks the bound) into host buffers laid out as k_acc_paths writes them; one synchronise per ACC_BATCH
  int paths(AccErr e, hipStream_t s, const uint64_t *idx, uint32_t nidx, uint64_t *siblings, uint32_t *path_bits,
            uint32_t *depth, uint64_t *leaves);
  // roots_out[i][4] (host) = the root the tree had at ms[i] leaves (host; each in 1..n(), the caller checks
  // the bound before anything is enqueued); one synchronise per ACC_BATCH
  int prefix_roots(AccErr e, hipStream_t s, const uint64_t *ms, uint32_t k, uint64_t *roots_out);
  // the same leaves re-laid for new_capacity, nlv = their table there: a new buffer beside the old, every
  // level copied, the stream synchronised; the tree moves over only once all of it succeeded
  int reserve(AccErr e, uint64_t new_capacity, const qpk::AccLevels &nlv, hipStream_t s);
};

// The prefix roots that an audit's commitment claims (root_i, n_i) name, fetched from `tree` (n
// leaves) in one batch by the first get(), so a verdict that stops at an earlier reason launches
// nothing: get(i, out) = the root at n_i leaves, for a claim with n_i <= n.  rc: what the batch
// returned (its reason is in e.err).
struct PrefixRootBatch {
  AccTree &tree;
  AccErr e;
  hipStream_t s;
  const uint64_t *ns;  // [k]
  uint32_t k;
  uint64_t n;
  int rc = 0;  // QP_OK
  bool asked = false;
  std::vector<uint64_t> ms, got;
  std::vector<uint32_t> at;
  void get(uint32_t i, uint64_t out[4]);
};
