"""The nullifier-set commitment (include/qpgpu.h qp_*_commit_set, qp_*_set_proofs,
qp_nullifier_set_*): a Merkle root over the *sorted* set of a handle's admitted
nullifiers, and proofs that a nullifier is, or is not, in it.

The log commitment (`commit_log`, receipts) proves what was admitted.  This one
proves what was not: absence of a key is two adjacent leaves of the sorted tree
that straddle it.  A BallotBox commits its counted nullifiers, a WormholeLedger
its credited ones; both share the definitions:

  order    the nullifier's four felts, felt 0 first, as unsigned 64-bit words,
           then the log index seq
  set leaf hash_no_pad([key[0..4], seq, 2]) at sorted position j
  set tree the log tree's kind (odd node promoted); commitment (root, m); m = 0
           has the zero root
  proof    pos = the set keys below the key, and found.  found: the leaf at pos
           (hi) has the key.  Not found: lo = the leaf at pos - 1 (None if pos
           is 0) is below the key, hi = the leaf at pos (None if pos is m) above.

With a Context the set is selected, sorted, hashed and searched on the device
(csrc/nullifier_set.hip); with None the same runs on the host.
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._native import QpError, lib

PATH_SLOTS = 32
NOT_FOUND = 2**64 - 1
# qp_nullifier_set_check: qp_receipt_status 0..4, then qp_set_status
SET_CHECK_TEXT = ("ok", "shape", "root", "non-canonical", "null", "order")

# one leaf of the set tree with its path: siblings are the `depth` digests from the leaf up
NullifierLeaf = namedtuple("NullifierLeaf", "key seq siblings path_bits depth")
# the proof for `key` under the commitment (root, m)
NullifierProof = namedtuple("NullifierProof", "key found pos lo hi root m")


def _query_keys(keys):
    if isinstance(keys, np.ndarray) and keys.dtype == np.uint64 and keys.ndim == 2 and keys.shape[1] == 4:
        return np.ascontiguousarray(keys)
    rows = [[int(x) for x in k] for k in keys]
    for i, r in enumerate(rows):
        if len(r) != 4 or any(not 0 <= x < 2**64 for x in r):
            raise ValueError(f"nullifier at position {i} must be 4 field elements")
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 4)


def nullifier_set_tile():
    """The records one workgroup of the device sort orders in LDS."""
    return int(lib().qp_nullifier_set_tile())


def nullifier_set_times():
    """Stage times (ms) of the last device build of a set on this thread, or None:
    select, tile sort (with the host's wait for m), duplicates + leaves, levels, and
    one figure per merge pass."""
    ms = (ctypes.c_double * 36)()
    n = lib().qp_nullifier_set_times(ms, 36)
    if not n:
        return None
    return {"select_ms": ms[0], "tile_sort_ms": ms[1], "leaves_ms": ms[2], "levels_ms": ms[3],
            "merge_pass_ms": [ms[4 + p] for p in range(n - 4)]}


def _members(entries):
    """(nullifiers [n][4], member [n] u8) of a published log: (nullifiers, member), a
    box's `entries()` 4-tuple or (nullifiers, numbers, flags), or a ledger's
    `entries()` 5-tuple (credited bools, or flag bytes)"""
    entries = tuple(entries)
    if len(entries) == 2:
        nul, mem = entries
        mem = np.asarray(mem) != 0
    elif len(entries) == 3:
        nul, mem = entries[0], (np.asarray(entries[2]).astype(np.uint8) & 2) != 0
    elif len(entries) == 4:
        nul, mem = entries[0], np.asarray(entries[2], dtype=bool)
    elif len(entries) == 5:
        fl = np.asarray(entries[4])
        nul, mem = entries[0], fl if fl.dtype == bool else (fl.astype(np.uint8) & 1) != 0
    else:
        raise ValueError("a log is (nullifiers, member), a box's entries or a ledger's entries")
    nul = np.ascontiguousarray(nul, dtype=np.uint64).reshape(-1, 4)
    mem = np.ascontiguousarray(mem, dtype=np.uint8).reshape(-1)
    if len(nul) != len(mem):
        raise ValueError(f"a log of {len(nul)} nullifiers and {len(mem)} member flags")
    return nul, mem


def nullifier_set_root(ctx_or_none, entries):
    """(root, m, order, duplicate): the set commitment of a published log, the members'
    seqs in sorted order, and None or the lowest seq of a member whose nullifier an
    earlier member holds.  `entries`: see `_members`.  An auditor compares (root, m)
    with what the operator published.  Needs no handle."""
    nul, mem = _members(entries)
    n = len(mem)
    root, m, dup = np.zeros(4, np.uint64), ctypes.c_uint64(), ctypes.c_uint64()
    order = np.zeros(max(n, 1), np.uint64)
    rc = lib().qp_nullifier_set_root(None if ctx_or_none is None else ctx_or_none.h, nul.ctypes.data, mem.ctypes.data, n,
                                     root.ctypes.data, ctypes.byref(m), order.ctypes.data, ctypes.byref(dup))
    if rc:
        raise QpError(rc, lib().qp_nullifier_set_last_error().decode())
    return ([int(x) for x in root], m.value, [int(x) for x in order[:m.value]],
            None if dup.value == NOT_FOUND else dup.value)


def _slot_arrays(leaf):
    """(key [4], seq, siblings [32][4], bits, depth) of a proof's slot for the checker; None: all zero"""
    sib = np.zeros((PATH_SLOTS, 4), np.uint64)
    if leaf is None:
        return np.zeros(4, np.uint64), 0, sib, 0, 0
    key = np.array([int(x) for x in leaf.key], dtype=np.uint64)
    if key.shape != (4,):
        raise ValueError("a key is 4 field elements")
    if leaf.siblings:
        sib[:len(leaf.siblings)] = np.array([[int(x) for x in d] for d in leaf.siblings], dtype=np.uint64)
    for v, bound in ((leaf.seq, 2**64), (leaf.path_bits, 2**32), (leaf.depth, 2**32)):
        if not 0 <= int(v) < bound:
            raise ValueError("a value that fits no field of a proof")
    return key, int(leaf.seq), sib, int(leaf.path_bits), int(leaf.depth)


def nullifier_proof_status(p, root=None, m=None):
    """The checker's code for proof `p` under (root, m), which default to the pair the
    proof names: 0 ok, else the first reason (SET_CHECK_TEXT)."""
    root = p.root if root is None else root
    m = p.m if m is None else m
    rt = np.array([int(x) for x in root], dtype=np.uint64)
    x = np.array([int(v) for v in p.key], dtype=np.uint64)
    if rt.shape != (4,) or x.shape != (4,):
        raise ValueError("root and key are 4 field elements each")
    if not (0 <= int(m) < 2**64 and 0 <= int(p.pos) < 2**64 and 0 <= int(p.found) < 2**32):
        raise ValueError("a value that fits no field of a proof")
    lk, ls, lsib, lb, ld = _slot_arrays(p.lo)
    hk, hs, hsib, hb, hd = _slot_arrays(p.hi)
    return lib().qp_nullifier_set_check(rt.ctypes.data, int(m), x.ctypes.data, int(p.found), int(p.pos), lk.ctypes.data,
                                        ls, lsib.ctypes.data, lb, ld, hk.ctypes.data, hs, hsib.ctypes.data, hb, hd)


def check_nullifier_proof(p, root=None, m=None):
    """True iff proof `p` holds under the published set commitment (root, m), which
    default to the pair the proof names.  A proof is valid only under the pair it was
    made under.  Needs no handle and no device."""
    try:
        return nullifier_proof_status(p, root, m) == 0
    except (OverflowError, ValueError, TypeError, IndexError):
        return False  # a value that fits no field of a proof


class NullifierSetMixin:
    """commit_nullifiers / nullifier_proofs of a handle; `_SET_ABI` names its C prefix."""

    def commit_nullifiers(self):
        """(root, m): the commitment to the sorted set of this handle's admitted
        nullifiers (a box's counted, a ledger's credited ones).  Rebuilt when an entry
        was admitted since the last call; an empty handle gives ([0, 0, 0, 0], 0)."""
        root, m = np.zeros(4, np.uint64), ctypes.c_uint64()
        self._check(getattr(lib(), self._SET_ABI + "_commit_set")(self.h, root.ctypes.data, ctypes.byref(m)))
        return [int(x) for x in root], m.value

    def nullifier_proofs(self, keys):
        """One NullifierProof per key (4 canonical felts each), all under one (root, m):
        membership if the key's nullifier was admitted, absence if not."""
        q = _query_keys(keys)
        k = len(q)
        found, pos = np.zeros(k, np.uint8), np.zeros(k, np.uint64)
        key = [np.zeros((k, 4), np.uint64) for _ in range(2)]
        seq = [np.zeros(k, np.uint64) for _ in range(2)]
        sib = [np.zeros((k, PATH_SLOTS, 4), np.uint64) for _ in range(2)]
        bits = [np.zeros(k, np.uint32) for _ in range(2)]
        depth = [np.zeros(k, np.uint32) for _ in range(2)]
        root, m = np.zeros(4, np.uint64), ctypes.c_uint64()
        args = [self.h, q.ctypes.data, k, found.ctypes.data, pos.ctypes.data]
        for s in range(2):
            args += [key[s].ctypes.data, seq[s].ctypes.data, sib[s].ctypes.data, bits[s].ctypes.data, depth[s].ctypes.data]
        self._check(getattr(lib(), self._SET_ABI + "_set_proofs")(*args, root.ctypes.data, ctypes.byref(m)))
        root, m = [int(x) for x in root], m.value

        def leaf(s, i):
            return NullifierLeaf([int(x) for x in key[s][i]], int(seq[s][i]), sib[s][i, :depth[s][i]].tolist(),
                                 int(bits[s][i]), int(depth[s][i]))

        out = []
        for i in range(k):
            f, p = bool(found[i]), int(pos[i])
            out.append(NullifierProof([int(x) for x in q[i]], f, p, leaf(0, i) if not f and p > 0 else None,
                                      leaf(1, i) if p < m else None, root, m))
        return out

    def nullifier_proof_for(self, key):
        return self.nullifier_proofs([key])[0]

    check_nullifier_proof = staticmethod(check_nullifier_proof)
