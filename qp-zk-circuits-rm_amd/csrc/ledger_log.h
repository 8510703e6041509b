// ledger_log.h — the transfer ledger's log commitment in host C++: the log's
// leaf and node hashes, the log tree of the host path (an accumulator tree,
// acc_layout.h's HostTree, with the ledger's leaf) and the receipt check (host
// code on both paths; it needs no ledger and no device).  Included by
// ledger.cpp, ledger_audit.h and the stand-alone check tools/ledger_log_check.cpp.
//
// Definitions (DESIGN §14 and qpgpu.h state the same):
//   log leaf of entry seq = hash_no_pad([nullifier[0..4], number, amount[0..4],
//     account[0..4], flags]): 14 felts.  amount is the four 32-bit limbs as the
//     log holds them, most significant first, each one felt; flags is the log's
//     byte (bit 0 credited).  In the overwrite sponge that is two permutations:
//     state = 0; felts 0..7 into state[0..8], permute; felts 8..13 into
//     state[0..6] with state[6..12] as the first permutation left them,
//     permute; the digest is state[0..4].
//   log tree over leaves [0, n), n = admitted: an accumulator tree
//     (acc_layout.h): node = hash_no_pad(left || right), the last node of an odd
//     level moves up unchanged; laid out for the ledger's capacity
//   commitment = (root, n); the settler publishes (root, n, payouts)
// The checker (qpk::receipt_walk) takes the tree's shape from (seq, n), never
// from the receipt.  A leaf is
// the second permutation of a sponge and a node the only permutation of one
// over a zero state, so a node's digest is a leaf's only where a 14-felt input
// and an 8-felt input collide.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "acc_layout.h"
#include "ledger_table.h"
#include "poseidon.h"

namespace ql {

constexpr uint32_t LEAF_FELTS = 14;
using qpk::ACC_PATH_SLOTS, qpk::RECEIPT_NON_CANONICAL, qpk::RECEIPT_NULL, qpk::RECEIPT_OK, qpk::RECEIPT_ROOT, qpk::RECEIPT_SHAPE;

inline void log_leaf(const uint64_t nul[4], uint64_t number, const uint32_t amount[4], const uint64_t account[4],
                     uint8_t flags, uint64_t out[4]) {
  uint64_t s[12] = {nul[0], nul[1], nul[2], nul[3], number, amount[0], amount[1], amount[2], 0, 0, 0, 0};
  ps::permute(s);
  s[0] = amount[3];
  for (int j = 0; j < 4; j++) s[1 + j] = account[j];
  s[5] = flags;
  ps::permute(s);
  memcpy(out, s, 32);
}

// the node hash, hash_no_pad(left || right): one function for every log tree
inline constexpr auto &log_node = ps::two_to_one;

// the host path's log tree: a qpk::HostTree laid out for the ledger's capacity, the log's entries its leaves
struct HostLog : qpk::HostTree {
  // level 0 for entries [first, end) of a log in SoA form.  false: a number >= p (cannot be reached)
  bool leaves(const uint64_t *nullifier, const uint64_t *number, const uint32_t *amount, const uint64_t *account,
              const uint8_t *flags, uint64_t first, uint64_t end) {
    for (uint64_t seq = first; seq < end; seq++) {
      if (number[seq] >= P) return false;
      log_leaf(nullifier + seq * 4, number[seq], amount + seq * 4, account + seq * 4, flags[seq], node(0, seq));
    }
    return true;
  }
  // brings the tree up to the ledger's log: leaves [n, count), then the nodes above.  A tree laid out
  // for another capacity (the ledger was reserved) is rebuilt.  false: a number >= p in the log; the
  // tree is then dropped.
  bool commit(const HostLedger &h) {
    const uint64_t count = h.count();
    if (capacity != h.capacity) open(h.capacity);
    if (n == count) return true;
    if (!leaves(h.nullifier.data(), h.number.data(), h.amount.data(), h.account.data(), h.flags.data(), n, count)) {
      drop();
      return false;
    }
    append(count, log_node);
    return true;
  }
};

// qp_ledger_receipt_check: RECEIPT_OK or the first reason found, in this order: a felt >= p (or a
// flags byte above 1), the shape, the root.  An amount limb is in range by its type.
inline int receipt_check(const uint64_t root[4], uint64_t n, uint64_t seq, const uint64_t nullifier[4], uint64_t number,
                         const uint32_t amount[4], const uint64_t account[4], uint8_t flags, const uint64_t *siblings,
                         uint32_t path_bits, uint32_t depth) {
  if (!canonical(nullifier, 4) || number >= P || !canonical(account, 4) || flags > FLAG_CREDITED)
    return RECEIPT_NON_CANONICAL;
  uint64_t leaf[4];
  log_leaf(nullifier, number, amount, account, flags, leaf);
  return qpk::receipt_walk(root, n, seq, leaf, siblings, path_bits, depth, log_node);
}

}  // namespace ql
