// claims.h — the payout claims commitment in host C++ (no HIP beyond QL_HD):
// the order, the five-limb total, the claim leaf, the host path (std::sort on
// the rows of a payout round, then an accumulator tree, acc_layout.h's
// HostTree) and the checker of a claim (host code on both paths; it needs no
// ledger and no device).  Included by claims_commit.h, claims.cpp, claims.hip
// (the device leaves normalise with the statement below) and the stand-alone
// check tools/claims_check.cpp.
//
// Definitions (DESIGN §17 and qpgpu.h state the same).  For a log range [m0,
// m1), 0 <= m0 <= m1 <= admitted:
//   rows     = exactly the rows qp_ledger_payouts_between(m0, m1) gives, A of
//              them: an account, four limb sums and first_seq (the lowest
//              credited seq of the account in the range, counted from 0 in the
//              whole log).
//   order    = by account, as ql::key_compare compares its four felts (felt 0
//              first, each a full unsigned 64-bit word), with qns::rec_less,
//              the nullifier set's comparator, first_seq as the fifth word.
//              Accounts are distinct within a range by construction.
//   total of a row: T = sum_i sums[i] << (96 - 32 i), carry-normalised into
//              five 32-bit limbs t[0..5), most significant first.  A range
//              holds at most 2^31 entries of at most 2^128 each: T < 2^160.
//   claim leaf at sorted position j = hash_no_pad([account[0..4], t[0..5],
//              first_seq, 3]): 11 felts, two permutations of the overwrite
//              sponge, as the ledger's 14-felt log leaf: felts 0..7 into
//              state[0..8], permute; felts 8..10 into state[0..3] with
//              state[3..12] kept, permute; the digest is state[0..4].
//   claims tree over leaves [0, A): an accumulator tree, node =
//              hash_no_pad(left || right), the odd node promoted.
//   commitment = (claims_root, A, total[5]) for the named (m0, m1); total =
//              the five-limb sum of all rows.  A = 0: the zero root, a zero
//              total, and every absence holds with no path.
//   claim for account x: pos = the number of rows with an account below x, and
//              found.  Found: the leaf at pos (the `hi` slot) has account x and
//              its total is what x is owed.  Not found: the leaf at pos - 1
//              (`lo`, pos > 0) is below x and the leaf at pos (`hi`, pos < A)
//              above.  A slot the proof has no use for is all zero.
// The checker takes the tree's shape from (j, A) alone, as qns::check does.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "acc_layout.h"
#include "ledger_rounds.h"
#include "ledger_table.h"
#include "nullifier_set.h"
#include "poseidon.h"

namespace qcl {

using ql::key_compare, qst::canonical, qst::key_equal, qst::P;
using qpk::ACC_MAX_LEAVES, qpk::ACC_PATH_SLOTS, qpk::RECEIPT_NON_CANONICAL, qpk::RECEIPT_NULL, qpk::RECEIPT_OK,
    qpk::RECEIPT_ROOT, qpk::RECEIPT_SHAPE;
using qns::SET_ORDER;
constexpr uint64_t LEAF_TAG = 3;  // felt 10 of a claim leaf
constexpr uint32_t LIMBS = 5;

// Four limb sums (sums[i] weighs 2^(96 - 32 i)) into five 32-bit limbs, most significant first.
// Each sum is below 2^63 (at most 2^31 entries of limbs below 2^32) and a carry below 2^32, so
// sums[i] + carry does not wrap; the last carry is below 2^31 + 1 and is limb 0.
QL_HD inline void normalise(const uint64_t sums[4], uint32_t t[5]) {
  uint64_t carry = 0;
  for (int i = 3; i >= 0; i--) {
    const uint64_t v = sums[i] + carry;
    t[i + 1] = (uint32_t)v;
    carry = v >> 32;
  }
  t[0] = (uint32_t)carry;
}

inline void claim_leaf(const uint64_t account[4], const uint32_t t[5], uint64_t first_seq, uint64_t out[4]) {
  uint64_t s[12] = {account[0], account[1], account[2], account[3], t[0], t[1], t[2], t[3], 0, 0, 0, 0};
  ps::permute(s);
  s[0] = t[4];
  s[1] = first_seq;
  s[2] = LEAF_TAG;
  ps::permute(s);
  memcpy(out, s, 32);
}

inline constexpr auto &claim_node = ps::two_to_one;

// one slot of a claim: the leaf (account, total, first_seq) and its path in HostTree::path's layout
struct Slot {
  const uint64_t *account;  // [4]
  const uint32_t *total;    // [5]
  uint64_t first_seq;
  const uint64_t *siblings;  // [ACC_PATH_SLOTS][4]
  uint32_t path_bits, depth;
};

// the host path's claims: the sorted rows and the tree over their leaves
struct HostClaims {
  std::vector<uint64_t> accounts;   // [A][4], sorted
  std::vector<uint32_t> totals;     // [A][5]
  std::vector<uint64_t> first_seq;  // [A]
  qpk::HostTree tree;               // laid out for A leaves (A > 0)
  uint64_t root[4] = {0, 0, 0, 0};
  uint32_t total[5] = {0, 0, 0, 0, 0};

  uint64_t count() const { return first_seq.size(); }
  void drop() { *this = HostClaims(); }

  // from the rows of a payout round (ql::round_payouts_host).  The grand total's four limb sums are
  // each the sum of that limb over the range's credited entries: below 2^63, no wrap.
  void build(const ql::RoundRows &rows) {
    drop();
    const uint64_t A = rows.count();
    std::vector<uint32_t> at(A);
    for (uint64_t i = 0; i < A; i++) at[i] = (uint32_t)i;
    std::sort(at.begin(), at.end(), [&rows](uint32_t a, uint32_t b) {
      return qns::rec_less(&rows.accounts[(size_t)a * 4], rows.first_seq[a], &rows.accounts[(size_t)b * 4], rows.first_seq[b]);
    });
    accounts.resize(A * 4), totals.resize(A * LIMBS), first_seq.resize(A);
    uint64_t grand[4] = {0, 0, 0, 0};
    for (uint64_t j = 0; j < A; j++) {
      const uint64_t *sums = &rows.sums[(size_t)at[j] * 4];
      memcpy(&accounts[j * 4], &rows.accounts[(size_t)at[j] * 4], 32);
      first_seq[j] = rows.first_seq[at[j]];
      normalise(sums, &totals[j * LIMBS]);
      for (int i = 0; i < 4; i++) grand[i] += sums[i];
    }
    normalise(grand, total);
    if (!A) return;
    tree.open(A);
    for (uint64_t j = 0; j < A; j++) claim_leaf(&accounts[j * 4], &totals[j * LIMBS], first_seq[j], tree.node(0, j));
    tree.append(A, claim_node);
    memcpy(root, tree.root(), 32);
  }

  // pos and found of account x
  uint64_t search(const uint64_t x[4], bool *found) const {
    const uint64_t pos = qns::lower_bound(accounts.data(), count(), x);
    *found = pos < count() && key_equal(&accounts[pos * 4], x);
    return pos;
  }
};

inline bool slot_is_zero(const Slot &s) {
  if (s.first_seq || s.path_bits || s.depth || s.account[0] || s.account[1] || s.account[2] || s.account[3]) return false;
  for (uint32_t i = 0; i < LIMBS; i++)
    if (s.total[i]) return false;
  for (uint32_t i = 0; i < ACC_PATH_SLOTS * 4; i++)
    if (s.siblings[i]) return false;
  return true;
}

// qp_ledger_claim_check: RECEIPT_OK or the first reason found, in qns::check's order: a felt >= p
// (root, x, an account, first_seq, the siblings), the shape, the order, the root.  Shape: count >
// 2^31, pos > count, found > 1, found with pos = count, a path whose depth or side bits are not
// the ones (j, count) gives, a slot the proof has no use for that is not all zero (lo: pos = 0 or
// found; hi: pos = count).  Order: not lo.account < x < hi.account, or found with an account other
// than x.  Total limbs are in range by type.
inline int check(const uint64_t root[4], uint64_t count, const uint64_t x[4], uint32_t found, uint64_t pos, const Slot &lo,
                 const Slot &hi) {
  if (!canonical(root, 4) || !canonical(x, 4) || !canonical(lo.account, 4) || !canonical(hi.account, 4) ||
      lo.first_seq >= P || hi.first_seq >= P || !canonical(lo.siblings, ACC_PATH_SLOTS * 4) ||
      !canonical(hi.siblings, ACC_PATH_SLOTS * 4))
    return RECEIPT_NON_CANONICAL;
  if (count > ACC_MAX_LEAVES || pos > count || found > 1 || (found && pos == count)) return RECEIPT_SHAPE;
  const bool has_lo = !found && pos > 0, has_hi = pos < count;
  const Slot *slots[2] = {&lo, &hi};
  const bool has[2] = {has_lo, has_hi};
  const uint64_t at[2] = {pos - 1, pos};
  for (int i = 0; i < 2; i++) {
    if (!has[i]) {
      if (!slot_is_zero(*slots[i])) return RECEIPT_SHAPE;
      continue;
    }
    uint32_t d, b;
    qns::path_shape(at[i], count, &d, &b);
    if (slots[i]->depth != d || slots[i]->path_bits != b) return RECEIPT_SHAPE;
  }
  if (found) {
    if (!key_equal(hi.account, x)) return SET_ORDER;
  } else {
    if (has_lo && key_compare(lo.account, x) >= 0) return SET_ORDER;
    if (has_hi && key_compare(x, hi.account) >= 0) return SET_ORDER;
  }
  if (!count) return root[0] | root[1] | root[2] | root[3] ? RECEIPT_ROOT : RECEIPT_OK;
  for (int i = 0; i < 2; i++) {
    if (!has[i]) continue;
    uint64_t leaf[4];
    claim_leaf(slots[i]->account, slots[i]->total, slots[i]->first_seq, leaf);
    if (int rc = qpk::receipt_walk(root, count, at[i], leaf, slots[i]->siblings, slots[i]->path_bits, slots[i]->depth,
                                   claim_node))
      return rc;
  }
  return RECEIPT_OK;
}

}  // namespace qcl
