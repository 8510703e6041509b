// ballot_log.h — the ballot box's log commitment in host C++: the read-only
// lookup in the host table, the log's leaf and node hashes, the log tree of the
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
// The checker takes the tree's shape from (seq, n), never from the receipt
// (qpk::path_levels: at level l node j = seq >> l has a sibling iff (j ^ 1) <
// ceil(n / 2^l)), and a receipt whose depth or side bits say otherwise is
// rejected.  A six-felt leaf hashes as the eight-felt node (nullifier ||
// number, flags, 0, 0) would, so without this a node whose right child has
// that form could be offered as a leaf.  (depth, side bits) is the route from the root to one node of the tree,
// and the shape rule yields the routes of level-0 nodes only.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "acc_layout.h"
#include "ballot_table.h"
#include "poseidon.h"

namespace qb {

constexpr uint64_t NOT_FOUND = ~0ull;
constexpr uint32_t PATH_SLOTS = qpk::ACC_PATH_SLOTS;
// qp_receipt_status (qpgpu.h)
enum : int { RECEIPT_OK = 0, RECEIPT_SHAPE = 1, RECEIPT_ROOT = 2, RECEIPT_NON_CANONICAL = 3, RECEIPT_NULL = 4 };

// hash_no_pad of n <= 8 felts
inline void hash8(const uint64_t *in, uint32_t n, uint64_t out[4]) {
  uint64_t s[12] = {0};
  for (uint32_t i = 0; i < n; i++) s[i] = in[i];
  ps::permute(s);
  memcpy(out, s, 32);
}

inline void log_leaf(const uint64_t nul[4], uint64_t number, uint8_t flags, uint64_t out[4]) {
  const uint64_t in[6] = {nul[0], nul[1], nul[2], nul[3], number, flags};
  hash8(in, 6, out);
}

inline void log_node(const uint64_t l[4], const uint64_t r[4], uint64_t out[4]) {
  const uint64_t in[8] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3]};
  hash8(in, 8, out);
}

// the log index of the counted entry with nullifier q, NOT_FOUND if none: the
// table's probe without the claim.  An empty slot ends the chain (nothing is
// ever removed, so no chain has a gap); bounded by S like the insert's probe.
inline uint64_t find(const HostBox &b, const uint64_t q[4]) {
  uint64_t at = home_slot(q, b.mask);
  for (uint64_t tried = 0; tried <= b.mask; tried++, at = (at + 1) & b.mask) {
    const uint32_t cur = b.slot[at];
    if (cur == EMPTY) return NOT_FOUND;
    if (!memcmp(&b.nullifier[(size_t)cur * 4], q, 32)) return cur;
  }
  return NOT_FOUND;
}

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
  if (!canonical(root, 4) || !canonical(nullifier, 4) || number >= P || flags > (FLAG_VOTE | FLAG_COUNTED) ||
      !canonical(siblings, PATH_SLOTS * 4))
    return RECEIPT_NON_CANONICAL;
  if (!n || n > qpk::ACC_MAX_LEAVES || seq >= n) return RECEIPT_SHAPE;
  const uint32_t m = qpk::path_levels(seq, n);
  uint32_t d = 0, bits = 0;
  for (uint32_t l = 0; l < 32; l++)
    if (m >> l & 1) bits |= (uint32_t)((seq >> l) & 1) << d++;
  if (d != depth || bits != path_bits) return RECEIPT_SHAPE;
  for (uint32_t i = d * 4; i < PATH_SLOTS * 4; i++)
    if (siblings[i]) return RECEIPT_SHAPE;  // the slots above the depth hold the zero digest
  uint64_t cur[4];
  log_leaf(nullifier, number, flags, cur);
  for (uint32_t i = 0; i < d; i++) {
    const uint64_t *s = siblings + i * 4;
    if (bits >> i & 1)
      log_node(s, cur, cur);
    else
      log_node(cur, s, cur);
  }
  return memcmp(cur, root, 32) ? RECEIPT_ROOT : RECEIPT_OK;
}

}  // namespace qb
