// ballot_log.h — the ballot box's log commitment in host C++: the log's leaf
// and node hashes, the log tree of the
// host path (an accumulator tree, acc_layout.h's HostTree, with the log's leaf), and
// the receipt check (host code on both paths; it needs no box and no device).
// Included by ballot.cpp and by the stand-alone check tools/ballot_log_check.cpp.
//
// Definitions (DESIGN §13 and qpgpu.h state the same):
//   log leaf of entry seq = hash_no_pad([nullifier[0..4], number, flags]): six
//     felts, one permutation; flags is the log's byte (bit 0 vote, bit 1 counted)
//   log tree over leaves [0, n), n = admitted: an accumulator tree
//     (acc_layout.h): node = hash_no_pad(left || right), the last node of an odd
//     level moves up unchanged; laid out for the box's capacity, so it grows in
//     place
//   commitment = (root, n)
// The checker (qpk::receipt_walk) takes the tree's shape from (seq, n), never
// from the receipt.  A six-felt leaf hashes as the eight-felt node (nullifier ||
// number, flags, 0, 0) would, so without this a node whose right child has
// that form could be offered as a leaf.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "acc_layout.h"
#include "ballot_table.h"
#include "poseidon.h"

namespace qb {

using qpk::ACC_PATH_SLOTS, qpk::RECEIPT_NON_CANONICAL, qpk::RECEIPT_NULL, qpk::RECEIPT_OK, qpk::RECEIPT_ROOT, qpk::RECEIPT_SHAPE;

inline void log_leaf(const uint64_t nul[4], uint64_t number, uint8_t flags, uint64_t out[4]) {
  uint64_t s[12] = {nul[0], nul[1], nul[2], nul[3], number, flags, 0, 0, 0, 0, 0, 0};
  ps::permute(s);
  memcpy(out, s, 32);
}

// the node hash, hash_no_pad(left || right): one function for every log tree
inline constexpr auto &log_node = ps::two_to_one;

// the host path's log tree: a qpk::HostTree laid out for the box's capacity, the log's entries its leaves
struct HostLog : qpk::HostTree {
  // brings the tree up to the box's log: leaves [n, count), then the nodes above.  A tree laid out
  // for another capacity (the box was reserved) is rebuilt.  false: a number >= p in the log
  // (cannot be reached); the tree is then dropped.
  bool commit(const HostBox &b) {
    const uint64_t count = b.count();
    if (capacity != b.capacity) open(b.capacity);
    if (n == count) return true;
    for (uint64_t seq = n; seq < count; seq++) {
      if (b.number[seq] >= P) {
        drop();
        return false;
      }
      log_leaf(&b.nullifier[(size_t)seq * 4], b.number[seq], b.flags[seq], node(0, seq));
    }
    append(count, log_node);
    return true;
  }
};

// qp_ballot_receipt_check: RECEIPT_OK or the first reason found, in this
// order: a felt >= p (or a flags byte above 3), the shape, the root
inline int receipt_check(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t nullifier[4], uint64_t number,
                         uint8_t flags, const uint64_t *siblings, uint32_t path_bits, uint32_t depth) {
  if (!canonical(nullifier, 4) || number >= P || flags > (FLAG_VOTE | FLAG_COUNTED)) return RECEIPT_NON_CANONICAL;
  uint64_t leaf[4];
  log_leaf(nullifier, number, flags, leaf);
  return qpk::receipt_walk(root, n, seq, leaf, siblings, path_bits, depth, log_node);
}

}  // namespace qb
