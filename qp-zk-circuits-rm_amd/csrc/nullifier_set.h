// nullifier_set.h — the nullifier-set commitment in host C++ (no HIP): the
// order, the set leaf, the host path (std::sort, then an accumulator tree,
// acc_layout.h's HostTree) and the checker of a membership / absence proof (host
// code on both paths; it needs no handle and no device).  Included by
// set_commit.h, nullifier_set.cpp and the stand-alone check
// tools/nullifier_set_check.cpp; the device kernels (nullifier_set.hip) use the
// order from here, so both paths compare with one statement.
//
// Definitions (DESIGN §16 and qpgpu.h state the same; the ballot box and the
// transfer ledger share them):
//   set      = the entries of the log whose member flag is set (a box's counted
//              bit, a ledger's credited bit); m = their number.  By the handles'
//              invariant these are the distinct admitted nullifiers.
//   order    = ql::key_compare on the nullifier (four felts, felt 0 first, each a
//              full 64-bit unsigned word), then the log index seq as a fifth,
//              least significant word: total even on a malformed published log.
//   set leaf at sorted position j = hash_no_pad([K_j[0..4], seq_j, 2]): six felts,
//              one permutation
//   set tree over leaves [0, m): an accumulator tree (acc_layout.h) with the
//              log's node hash (ps::two_to_one), the odd node promoted
//   commitment = (set_root, m); m = 0: the root is four zeros
//   proof for a key x: pos = the number of set keys below x, and `found`.
//              found: the leaf at pos has key x (the `hi` slot).  Not found: the
//              leaf at pos - 1 (pos > 0; the `lo` slot) has a key below x and the
//              leaf at pos (pos < m; the `hi` slot) a key above x.  The two
//              positions are adjacent, so nothing lies between them.
// The checker (qpk::receipt_walk) takes the tree's shape from (j, m), never from
// the proof.  A set leaf hashes as the eight-felt node (K || seq, 2, 0, 0)
// would, and a box's log leaf (nullifier || number, flags <= 3) has the same
// form: the constant 2 in felt 5 does not keep them apart, the position in the
// tree does.  A path's (depth, side bits) is the route from the root to one node;
// path_levels yields the routes of level-0 nodes only, and a proof that says
// otherwise is rejected, so a node (or a leaf of another tree under another
// root) cannot be offered as a set leaf.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "acc_layout.h"
#include "ledger_table.h"
#include "poseidon.h"

namespace qns {

using ql::key_compare, qst::canonical, qst::key_equal, qst::NOT_FOUND, qst::P;
using qpk::ACC_MAX_LEAVES, qpk::ACC_PATH_SLOTS, qpk::RECEIPT_NON_CANONICAL, qpk::RECEIPT_NULL, qpk::RECEIPT_OK,
    qpk::RECEIPT_ROOT, qpk::RECEIPT_SHAPE;
// qp_set_status (qpgpu.h): the one reason the set checker adds to a receipt's
enum : int { SET_ORDER = 5 };
constexpr uint64_t LEAF_TAG = 2;  // felt 5 of a set leaf

// the order: (key, seq) as five unsigned words
QL_HD inline bool rec_less(const uint64_t *ka, uint64_t sa, const uint64_t *kb, uint64_t sb) {
  const int c = key_compare(ka, kb);
  return c ? c < 0 : sa < sb;
}

inline void set_leaf(const uint64_t key[4], uint64_t seq, uint64_t out[4]) {
  uint64_t s[12] = {key[0], key[1], key[2], key[3], seq, LEAF_TAG, 0, 0, 0, 0, 0, 0};
  ps::permute(s);
  memcpy(out, s, 32);
}

inline constexpr auto &set_node = ps::two_to_one;

// keys [m][4] sorted: the number of keys below x (the first position whose key is not below x).
// Bounded by 32 halvings (m <= 2^31).
QL_HD inline uint64_t lower_bound(const uint64_t *keys, uint64_t m, const uint64_t *x) {
  uint64_t lo = 0, hi = m;
  for (int i = 0; i < 33 && lo < hi; i++) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (key_compare(keys + mid * 4, x) < 0) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one slot of a proof: the leaf (key, seq) and its path in HostTree::path's layout
struct Slot {
  const uint64_t *key;       // [4]
  uint64_t seq;
  const uint64_t *siblings;  // [ACC_PATH_SLOTS][4]
  uint32_t path_bits, depth;
};

// the host path's set: the sorted records and the tree over their leaves
struct HostSet {
  std::vector<uint64_t> keys;  // [m][4], sorted
  std::vector<uint32_t> seqs;  // [m]
  qpk::HostTree tree;          // laid out for m leaves (m > 0)
  uint64_t root[4] = {0, 0, 0, 0};
  uint64_t dup = NOT_FOUND;  // the lowest seq of a member whose key an earlier position holds

  uint64_t m() const { return seqs.size(); }
  void drop() { *this = HostSet(); }

  // The set of log [0, n): the entries with flags[seq] & mask, their keys from nullifiers[n][4].
  // n <= 2^31 and every member key canonical (the caller checks).
  void build(const uint64_t *nullifiers, const uint8_t *flags, uint64_t n, uint8_t mask) {
    drop();
    for (uint64_t seq = 0; seq < n; seq++)
      if (flags[seq] & mask) seqs.push_back((uint32_t)seq);
    std::sort(seqs.begin(), seqs.end(), [nullifiers](uint32_t a, uint32_t b) {
      return rec_less(nullifiers + (size_t)a * 4, a, nullifiers + (size_t)b * 4, b);
    });
    const uint64_t cnt = m();
    keys.resize(cnt * 4);
    for (uint64_t j = 0; j < cnt; j++) memcpy(&keys[j * 4], nullifiers + (size_t)seqs[j] * 4, 32);
    for (uint64_t j = 1; j < cnt; j++)
      if (key_equal(&keys[j * 4], &keys[(j - 1) * 4])) dup = std::min<uint64_t>(dup, seqs[j]);
    if (!cnt) return;
    tree.open(cnt);
    for (uint64_t j = 0; j < cnt; j++) set_leaf(&keys[j * 4], seqs[j], tree.node(0, j));
    tree.append(cnt, set_node);
    memcpy(root, tree.root(), 32);
  }

  // pos and found of key x
  uint64_t search(const uint64_t x[4], bool *found) const {
    const uint64_t pos = lower_bound(keys.data(), m(), x);
    *found = pos < m() && key_equal(&keys[pos * 4], x);
    return pos;
  }
};

// what (j, m) says a path looks like: the depth and the side bits (j < m <= 2^31)
inline void path_shape(uint64_t j, uint64_t m, uint32_t *depth, uint32_t *bits) {
  const uint32_t lv = qpk::path_levels(j, m);
  uint32_t d = 0, b = 0;
  for (uint32_t l = 0; l < 32; l++)
    if (lv >> l & 1) b |= (uint32_t)((j >> l) & 1) << d++;
  *depth = d;
  *bits = b;
}

inline bool slot_is_zero(const Slot &s) {
  if (s.seq || s.path_bits || s.depth || s.key[0] || s.key[1] || s.key[2] || s.key[3]) return false;
  for (uint32_t i = 0; i < ACC_PATH_SLOTS * 4; i++)
    if (s.siblings[i]) return false;
  return true;
}

// qp_nullifier_set_check: RECEIPT_OK or the first reason found, in this order: a felt >= p, the
// shape, the order, the root.  Shape: m > 2^31, pos > m, found > 1, found with pos = m, a path whose
// depth or side bits are not the ones (j, m) gives, a slot the proof has no use for that is not all
// zero (lo: pos = 0 or found; hi: pos = m).  Order: not lo.key < x < hi.key, or found with a key
// other than x.
inline int check(const uint64_t root[4], uint64_t m, const uint64_t x[4], uint32_t found, uint64_t pos, const Slot &lo,
                 const Slot &hi) {
  if (!canonical(root, 4) || !canonical(x, 4) || !canonical(lo.key, 4) || !canonical(hi.key, 4) || lo.seq >= P ||
      hi.seq >= P || !canonical(lo.siblings, ACC_PATH_SLOTS * 4) || !canonical(hi.siblings, ACC_PATH_SLOTS * 4))
    return RECEIPT_NON_CANONICAL;
  if (m > ACC_MAX_LEAVES || pos > m || found > 1 || (found && pos == m)) return RECEIPT_SHAPE;
  const bool has_lo = !found && pos > 0, has_hi = pos < m;
  const Slot *slots[2] = {&lo, &hi};
  const bool has[2] = {has_lo, has_hi};
  const uint64_t at[2] = {pos - 1, pos};
  for (int i = 0; i < 2; i++) {
    if (!has[i]) {
      if (!slot_is_zero(*slots[i])) return RECEIPT_SHAPE;
      continue;
    }
    uint32_t d, b;
    path_shape(at[i], m, &d, &b);
    if (slots[i]->depth != d || slots[i]->path_bits != b) return RECEIPT_SHAPE;
  }
  if (found) {
    if (!key_equal(hi.key, x)) return SET_ORDER;
  } else {
    if (has_lo && key_compare(lo.key, x) >= 0) return SET_ORDER;
    if (has_hi && key_compare(x, hi.key) >= 0) return SET_ORDER;
  }
  if (!m) return root[0] | root[1] | root[2] | root[3] ? RECEIPT_ROOT : RECEIPT_OK;
  for (int i = 0; i < 2; i++) {
    if (!has[i]) continue;
    uint64_t leaf[4];
    set_leaf(slots[i]->key, slots[i]->seq, leaf);
    if (int rc = qpk::receipt_walk(root, m, at[i], leaf, slots[i]->siblings, slots[i]->path_bits, slots[i]->depth, set_node))
      return rc;
  }
  return RECEIPT_OK;
}

}  // namespace qns
