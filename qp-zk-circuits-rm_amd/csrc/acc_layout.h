// acc_layout.h — the host-only half of the accumulator tree, the Merkle tree
// that the voter registry (eligibility) and the ballot box (its log) both keep
// (acc_kernels.h has the convention): the level table, the layout reserved for
// a capacity, the dirty ranges of an append, the shape rule of a path, the tree
// in host memory, the walk that checks a receipt, and the sorted batch of a
// registry's replace.  Plain C++ (no HIP, no hash): tools/acc_layout_check.cpp runs it under the sanitizers.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "slot_table.h"

namespace qpk {

// the voting circuit has MAX_MERKLE_DEPTH = 32 sibling slots and a 5-bit depth
// split: the deepest path a tree may hold is 31 (N <= 2^31)
constexpr uint32_t ACC_PATH_SLOTS = 32, ACC_MAX_DEPTH = 31, ACC_MAX_LEVELS = ACC_MAX_DEPTH + 1;
constexpr uint64_t ACC_MAX_LEAVES = (uint64_t)1 << ACC_MAX_DEPTH;
// from a level of at most this many nodes up, the rest of the tree is one launch
constexpr uint32_t ACC_FOLD_MAX = 64;

// level offsets (in digests) and lengths, leaves first; the root is level nlevels - 1
struct AccLevels {
  uint32_t nlevels = 0;
  uint64_t off[ACC_MAX_LEVELS] = {0}, len[ACC_MAX_LEVELS] = {0};
  uint64_t total() const { return nlevels ? off[nlevels - 1] + len[nlevels - 1] : 0; }
  uint32_t max_depth() const { return nlevels - 1; }
};

// the table of n leaves in a layout for `capacity` leaves: off[] from the
// capacity (every level the capacity can reach, so the tree grows in place),
// len[] and nlevels from n (n = 0: no levels).  With capacity == n the levels
// are dense: total() == acc_reserved(n).  false (table untouched) unless
// n <= capacity, 1 <= capacity <= 2^31.
inline bool acc_levels_reserved(uint64_t n, uint64_t capacity, AccLevels &lv) {
  if (!capacity || capacity > ACC_MAX_LEAVES || n > capacity) return false;
  AccLevels t;
  uint64_t o = 0;
  uint32_t l = 0;
  for (uint64_t len = capacity;; len = (len + 1) / 2) {
    t.off[l++] = o;
    o += len;
    if (len == 1) break;
  }
  for (uint64_t len = n; len; len = (len + 1) / 2) {
    t.len[t.nlevels++] = len;
    if (len == 1) break;
  }
  lv = t;
  return true;
}

// the digests a layout for `capacity` leaves reserves: level l holds
// ceil(capacity / 2^l) of them, down to the one root (0 for capacity 0 or > 2^31)
inline uint64_t acc_reserved(uint64_t capacity) {
  AccLevels full;
  return acc_levels_reserved(capacity, capacity, full) ? full.total() : 0;
}

// nodes [first, end) of one level
struct AccRange {
  uint64_t first = 0, end = 0;
};

// the nodes of every level that an append from n_old to n_new > n_old leaves
// changes: level l's are [n_old >> l, ceil(n_new / 2^l)), one contiguous range
// whose source pairs start at 2 (n_old >> l), pair-aligned; a promoted lone
// last node lies inside it.  Returns the level count of n_new.
inline uint32_t acc_append_ranges(uint64_t n_old, uint64_t n_new, AccRange (&rg)[ACC_MAX_LEVELS]) {
  uint32_t l = 0;
  for (uint64_t len = n_new; len; len = (len + 1) / 2, l++) {
    rg[l].first = n_old >> l;
    rg[l].end = len;
    if (len == 1) {
      l++;
      break;
    }
  }
  return l;
}

// the tree's shape at leaf i of n, the one statement of the shape rule: bit l is set iff the node of
// leaf i at level l is hashed with a sibling, that is (i >> l) ^ 1 < ceil(n / 2^l) (i < n, 1 <= n <=
// 2^31).  A path holds one sibling per set bit, lowest level first.
inline uint32_t path_levels(uint64_t i, uint64_t n) {
  uint32_t m = 0, l = 0;
  for (uint64_t len = n; len > 1; len = (len + 1) / 2, l++)
    if (((i >> l) ^ 1) < len) m |= 1u << l;
  return m;
}

// the tree in host memory, laid out as the device keeps it.  What a leaf is, and the hash, are the owner's.
struct HostTree {
  uint64_t capacity = 0, n = 0;  // n: the leaves the levels above level 0 are made for
  AccLevels lv;                  // the table of n leaves
  std::vector<uint64_t> dig;     // [acc_reserved(capacity)][4]

  void drop() { *this = HostTree(); }
  // an empty tree for `capacity` leaves (1 <= capacity <= 2^31)
  void open(uint64_t cap) {
    drop();
    capacity = cap;
    acc_levels_reserved(0, cap, lv);
    dig.assign((size_t)acc_reserved(cap) * 4, 0);
  }
  uint64_t *node(uint32_t l, uint64_t j) { return &dig[(size_t)(lv.off[l] + j) * 4]; }
  const uint64_t *node(uint32_t l, uint64_t j) const { return &dig[(size_t)(lv.off[l] + j) * 4]; }
  const uint64_t *root() const { return node(lv.nlevels - 1, 0); }

  // level 0 is written for [n, n_new) (through node(0, i); n < n_new <= capacity): remakes the nodes
  // above that the append changes (acc_append_ranges).  hash(left, right, out): the node hash, out[4].
  template <class NodeHash>
  void append(uint64_t n_new, NodeHash hash) {
    acc_levels_reserved(n_new, capacity, lv);
    AccRange rg[ACC_MAX_LEVELS];
    const uint32_t nl = acc_append_ranges(n, n_new, rg);
    for (uint32_t l = 1; l < nl; l++)
      for (uint64_t j = rg[l].first; j < rg[l].end; j++) {
        if (2 * j + 1 < lv.len[l - 1])
          hash(node(l - 1, 2 * j), node(l - 1, 2 * j + 1), node(l, j));
        else
          memcpy(node(l, j), node(l - 1, 2 * j), 32);
      }
    n = n_new;
  }

  // leaf i < n: siblings [ACC_PATH_SLOTS][4] compacted (zero above the depth), side bits (bit j = 1: the
  // leaf's node is the right child), depth, the leaf digest (may be null): the layout qpk::acc_paths writes
  void path(uint64_t i, uint64_t *siblings, uint32_t *path_bits, uint32_t *depth, uint64_t *leaf) const {
    memset(siblings, 0, ACC_PATH_SLOTS * 32);
    uint32_t bits = 0, d = 0;
    for (uint32_t m = path_levels(i, n), l = 0; m >> l; l++) {
      if (!(m >> l & 1)) continue;
      const uint64_t j = i >> l;
      memcpy(siblings + d * 4, node(l, j ^ 1), 32);
      bits |= (uint32_t)(j & 1) << d++;
    }
    *path_bits = bits;
    *depth = d;
    if (leaf) memcpy(leaf, node(0, i), 32);
  }

  // the root the tree had when it held leaves [0, m), 1 <= m <= n: a fold from leaf m - 1 up.  At level l
  // the prefix has c = ceil(m / 2^l) nodes and the fold holds its last one: c odd, that node is promoted;
  // c even, its left sibling c - 2 covers only leaves below m, so it is the same digest in this larger
  // tree.  The layout qpk::acc_prefix_roots answers in.
  template <class NodeHash>
  void prefix_root(uint64_t m, NodeHash hash, uint64_t out[4]) const {
    memcpy(out, node(0, m - 1), 32);
    for (uint32_t l = 0;; l++) {
      const uint64_t c = (m + ((uint64_t)1 << l) - 1) >> l;
      if (c <= 1) return;
      if (!(c & 1)) hash(node(l, c - 2), out, out);
    }
  }
};

// qp_receipt_status (qpgpu.h)
enum : int { RECEIPT_OK = 0, RECEIPT_SHAPE = 1, RECEIPT_ROOT = 2, RECEIPT_NON_CANONICAL = 3, RECEIPT_NULL = 4 };

// The receipt of leaf seq (its digest `leaf`) against a commitment (root, n), siblings
// [ACC_PATH_SLOTS][4] in HostTree::path's layout: RECEIPT_OK or the first reason found, in this
// order: a felt >= p in the root or the siblings, the shape, the root.  The shape comes from (seq, n),
// never from the receipt: (depth, side bits) is the route from the root to one node of the tree,
// path_levels yields the routes of level-0 nodes only, and a receipt that says otherwise is
// rejected, so a node cannot be offered as a leaf.  hash(left, right, out): the node hash.
template <class NodeHash>
int receipt_walk(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t leaf[4], const uint64_t *siblings,
                 uint32_t path_bits, uint32_t depth, NodeHash hash) {
  if (!qst::canonical(root, 4) || !qst::canonical(siblings, ACC_PATH_SLOTS * 4)) return RECEIPT_NON_CANONICAL;
  if (!n || n > ACC_MAX_LEAVES || seq >= n) return RECEIPT_SHAPE;
  const uint32_t m = path_levels(seq, n);
  uint32_t d = 0, bits = 0;
  for (uint32_t l = 0; l < 32; l++)
    if (m >> l & 1) bits |= (uint32_t)((seq >> l) & 1) << d++;
  if (d != depth || bits != path_bits) return RECEIPT_SHAPE;
  for (uint32_t i = d * 4; i < ACC_PATH_SLOTS * 4; i++)
    if (siblings[i]) return RECEIPT_SHAPE;  // the slots above the depth hold the zero digest
  uint64_t cur[4];
  memcpy(cur, leaf, 32);
  for (uint32_t i = 0; i < d; i++) {
    const uint64_t *s = siblings + i * 4;
    if (bits >> i & 1)
      hash(s, cur, cur);
    else
      hash(cur, s, cur);
  }
  return memcmp(cur, root, 32) ? RECEIPT_ROOT : RECEIPT_OK;
}

// the order that sorts a replace batch by leaf index: order[b] = position in
// idx[] of the b-th smallest index.  false when an index is >= n (*bad = its
// position) or appears twice (*bad = the position of the second one in idx[]).
inline bool registry_replace_order(const uint64_t *idx, uint32_t k, uint64_t n, std::vector<uint32_t> &order,
                                   uint32_t *bad) {
  for (uint32_t b = 0; b < k; b++)
    if (idx[b] >= n) {
      *bad = b;
      return false;
    }
  order.resize(k);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(),
            [idx](uint32_t a, uint32_t b) { return idx[a] != idx[b] ? idx[a] < idx[b] : a < b; });
  for (uint32_t b = 1; b < k; b++)
    if (idx[order[b]] == idx[order[b - 1]]) {
      *bad = order[b];
      return false;
    }
  return true;
}

}  // namespace qpk
