"""Payout claims (include/qpgpu.h qp_ledger_commit_claims, qp_ledger_claims,
qp_ledger_log_claims_root, qp_ledger_claim_check): one Merkle root per payout
round over the per-account totals sorted by account, and a short proof per
payee, as a Merkle distributor works.

For a log range [m0, m1) the rows are those of `WormholeLedger.payouts_between`:

  order   by account: its four felts, felt 0 first, as unsigned 64-bit words
  total   the row's exact total, hashed as five 32-bit limbs, most significant
          first
  leaf    hash_no_pad([account[0..4], t[0..5], first_seq, 3]) at sorted position j
  tree    the log tree's kind (odd node promoted); the commitment is
          (root, count, total) for the named range; count = 0 has the zero root
  claim   pos = the rows with an account below the account, and found.  found:
          the leaf at pos (hi) is the account's and `total` is what it is owed.
          Not found: lo = the leaf at pos - 1 (None if pos is 0) is below the
          account, hi = the leaf at pos (None if pos is count) above: it is owed
          nothing in this round.

The types and the checker are here; the ledger's calls are WormholeLedger's
(`commit_claims`, `claims`, `claim_for`) and `ledger_log_claims_root`.
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._native import lib

PATH_SLOTS = 32
TOTAL_LIMBS = 5
# qp_ledger_claim_check: qp_receipt_status 0..4, then qp_set_status
CLAIM_CHECK_TEXT = ("ok", "shape", "root", "non-canonical", "null", "order")

# the commitment of range [m0, m1): total is the exact sum of every row's total
ClaimsCommitment = namedtuple("ClaimsCommitment", "root count total m0 m1")
# one leaf of the claims tree with its path: total is the account's exact total in the range,
# siblings the `depth` digests from the leaf up
ClaimLeaf = namedtuple("ClaimLeaf", "account total first_seq siblings path_bits depth")


class PayoutClaim(namedtuple("PayoutClaim", "account found pos lo hi root count m0 m1")):
    """The claim of `account` (4 felts) under the commitment (root, count) of range [m0, m1)."""
    __slots__ = ()

    @property
    def total(self):
        """what the account is owed in the range: its leaf's exact total, 0 if it is absent"""
        return self.hi.total if self.found and self.hi is not None else 0


def total_limbs(total):
    """an exact total as five 32-bit limbs, most significant first"""
    t = int(total)
    if not 0 <= t < 1 << 160:
        raise ValueError("a total is an int in [0, 2^160)")
    return [(t >> (128 - 32 * i)) & 0xFFFFFFFF for i in range(TOTAL_LIMBS)]


def limbs_total(limbs):
    return sum(int(v) << (128 - 32 * i) for i, v in enumerate(limbs))


def claims_times():
    """Stage times (ms) of the last device build of a claims tree on this thread, or
    None: credit + compaction (with the host's wait for the row count), tile sort,
    leaves + grand total, levels, and one figure per merge pass."""
    ms = (ctypes.c_double * 36)()
    n = lib().qp_ledger_claims_times(ms, 36)
    if not n:
        return None
    return {"credit_ms": ms[0], "tile_sort_ms": ms[1], "leaves_ms": ms[2], "levels_ms": ms[3],
            "merge_pass_ms": [ms[4 + p] for p in range(n - 4)]}


def _slot_arrays(leaf):
    """(account [4], total [5] u32, first_seq, siblings [32][4], bits, depth) of a claim's slot; None: all zero"""
    sib = np.zeros((PATH_SLOTS, 4), np.uint64)
    if leaf is None:
        return np.zeros(4, np.uint64), np.zeros(TOTAL_LIMBS, np.uint32), 0, sib, 0, 0
    acc = np.array([int(x) for x in leaf.account], dtype=np.uint64)
    if acc.shape != (4,):
        raise ValueError("an account is 4 field elements")
    tot = np.array(total_limbs(leaf.total), dtype=np.uint32)
    if leaf.siblings:
        sib[:len(leaf.siblings)] = np.array([[int(x) for x in d] for d in leaf.siblings], dtype=np.uint64)
    for v, bound in ((leaf.first_seq, 2**64), (leaf.path_bits, 2**32), (leaf.depth, 2**32)):
        if not 0 <= int(v) < bound:
            raise ValueError("a value that fits no field of a claim")
    return acc, tot, int(leaf.first_seq), sib, int(leaf.path_bits), int(leaf.depth)


def check_claim_status(p, root=None, count=None):
    """The checker's code for claim `p` under (root, count), which default to the pair
    the claim names: 0 ok, else the first reason (CLAIM_CHECK_TEXT)."""
    root = p.root if root is None else root
    count = p.count if count is None else count
    rt = np.array([int(x) for x in root], dtype=np.uint64)
    x = np.array([int(v) for v in p.account], dtype=np.uint64)
    if rt.shape != (4,) or x.shape != (4,):
        raise ValueError("root and account are 4 field elements each")
    if not (0 <= int(count) < 2**64 and 0 <= int(p.pos) < 2**64 and 0 <= int(p.found) < 2**32):
        raise ValueError("a value that fits no field of a claim")
    la, lt, ls, lsib, lb, ld = _slot_arrays(p.lo)
    ha, ht, hs, hsib, hb, hd = _slot_arrays(p.hi)
    return lib().qp_ledger_claim_check(rt.ctypes.data, int(count), x.ctypes.data, int(p.found), int(p.pos),
                                       la.ctypes.data, lt.ctypes.data, ls, lsib.ctypes.data, lb, ld,
                                       ha.ctypes.data, ht.ctypes.data, hs, hsib.ctypes.data, hb, hd)


def check_claim(p, root=None, count=None):
    """True iff claim `p` holds under the published claims commitment (root, count) of
    its round, which default to the pair the claim names.  A claim is valid only
    under the pair of its own range.  Needs no ledger and no device."""
    try:
        return check_claim_status(p, root, count) == 0
    except (OverflowError, ValueError, TypeError, IndexError):
        return False  # a value that fits no field of a claim
