"""BallotBox: the counter's side of an election (include/qpgpu.h qp_ballot_box_*).

A verified voting proof says only that some registered voter voted `vote` on
`proposal_id` under `merkle_root`, with this `nullifier`.  A box is opened for
one proposal with the roots the operator published; it verifies batches of
voting proofs through a WormholeVerifier of the voting circuit's data, screens
their 13 public inputs (proposal[0:4] root[4:8] vote[8] nullifier[9:13]) and
counts each nullifier once.  Every ballot cast gets a number, its position in
the stream of all ballots cast into the box, and a status, the first check it
fails (BALLOT_STATUS_TEXT, in the checks' order after "counted").  Of the
ballots with one nullifier the one with the lowest number is counted; the
others are double votes whose `first` names it.  Statuses and the tally depend
on the ballot stream alone, not on how it is cut into batches.

With a Context (or a device number) the nullifier set, the log of admitted
ballots and the tally live on the device (csrc/ballot.hip); with None the same
semantics run on the host.
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._native import Context, QpError, lib
from .nullifier_set import NullifierSetMixin
from .registry import PATH_SLOTS  # sibling slots of a receipt's path: the log tree is the registry's kind of tree

P = 0xFFFFFFFF00000001
NPI = 13
MAX_ROOTS = 64
MAX_CAPACITY = 1 << 31
DEFAULT_CAPACITY = 1024

# qp_ballot_status
COUNTED, PROOF_REJECTED, MALFORMED, WRONG_PROPOSAL, UNKNOWN_ROOT, BAD_VOTE, DOUBLE_VOTE = range(7)
BALLOT_STATUS_TEXT = ("counted", "proof rejected", "malformed public inputs", "wrong proposal", "unknown root",
                      "bad vote", "double vote")
FLAG_VOTE, FLAG_COUNTED = 1, 2

NOT_FOUND = 2**64 - 1       # qp_ballot_box_find: the nullifier was never admitted

BallotResult = namedtuple("BallotResult", "status verify_status number first")
# one log entry tied to a published commitment (root, n): siblings are the `depth` digests of the
# levels where the entry's node was hashed, from the leaf up; path_bits bit j = side of sibling j
BallotReceipt = namedtuple("BallotReceipt", "nullifier number vote counted seq siblings path_bits depth root n")
# qp_ballot_result
RESULT_DTYPE = np.dtype([("status", np.uint32), ("verify_status", np.uint32), ("number", np.uint64),
                         ("first", np.uint64)])


# qp_audit_status: the first reason that fires, in this order
(AUDIT_OK, AUDIT_NON_CANONICAL, AUDIT_ORDER, AUDIT_COUNT_RULE, AUDIT_TALLY, AUDIT_ROOT, AUDIT_COMMITMENT) = range(7)
AUDIT_STATUS_TEXT = ("ok", "non-canonical entry", "ballot numbers out of order", "count rule broken",
                     "claimed tally differs", "claimed root differs", "earlier commitment does not hold")
# the verdict on a published log: witness = the lowest offender (an entry's seq; for a commitment
# its index), first = the lowest seq holding the witness's nullifier (count rule only), None where
# there is none; root and (yes, no, counted) recomputed from the log (zero on a non-canonical one)
AuditReport = namedtuple("AuditReport", "status witness first root yes no counted")
# qp_audit_report
AUDIT_DTYPE = np.dtype([("status", np.uint32), ("pad", np.uint32), ("witness", np.uint64), ("first", np.uint64),
                        ("root", np.uint64, 4), ("yes", np.uint64), ("no", np.uint64), ("counted", np.uint64)])


def _digest(v, what):
    d = [int(x) for x in v]
    if len(d) != 4 or any(not 0 <= x < P for x in d):
        raise ValueError(f"{what} must be 4 canonical field elements")
    return np.array(d, dtype=np.uint64)


def _log_arrays(entries):
    """(nullifiers [n][4], numbers [n], flags [n]) of a published log: the 4-tuple
    `BallotBox.entries()` returns, or (nullifiers, numbers, flags bytes)"""
    entries = tuple(entries)
    if len(entries) == 4:
        nul, num, counted, votes = entries
        fl = (np.asarray(votes, dtype=bool).astype(np.uint8) * FLAG_VOTE
              + np.asarray(counted, dtype=bool).astype(np.uint8) * FLAG_COUNTED)
    elif len(entries) == 3:
        nul, num, fl = entries
    else:
        raise ValueError("a log is (nullifiers, numbers, counted, votes) or (nullifiers, numbers, flags)")
    nul = np.ascontiguousarray(nul, dtype=np.uint64).reshape(-1, 4)
    num = np.ascontiguousarray(num, dtype=np.uint64).reshape(-1)
    fl = np.ascontiguousarray(fl, dtype=np.uint8).reshape(-1)
    if not len(nul) == len(num) == len(fl):
        raise ValueError(f"a log of {len(nul)} nullifiers, {len(num)} numbers and {len(fl)} flags")
    return nul, num, fl


def audit_log(ctx_or_none, entries, root=None, tally=None, commitments=()):
    """Audits a published log against what was published beside it: `root` (4
    felts), `tally` (yes, no) and earlier `commitments` [(root_i, n_i), ...], each
    optional.  Returns an AuditReport whose status is the first reason that fires
    (AUDIT_STATUS_TEXT), with the lowest offender as the witness.  With a Context
    the audit runs on the device (csrc/ballot_audit.hip), with None on the host;
    it needs no box and does not alter the log."""
    nul, num, fl = _log_arrays(entries)
    r = None if root is None else np.array([int(x) for x in root], dtype=np.uint64)
    t = None if tally is None else np.array([int(x) for x in tally], dtype=np.uint64)
    if (r is not None and r.shape != (4,)) or (t is not None and t.shape != (2,)):
        raise ValueError("root is 4 field elements, tally is (yes, no)")
    commitments = list(commitments)
    cr = np.array([[int(x) for x in c[0]] for c in commitments], dtype=np.uint64).reshape(len(commitments), 4)
    cn = np.array([int(c[1]) for c in commitments], dtype=np.uint64)
    out = np.zeros(1, AUDIT_DTYPE)
    rc = lib().qp_ballot_log_audit(None if ctx_or_none is None else ctx_or_none.h, nul.ctypes.data, num.ctypes.data,
                                   fl.ctypes.data, len(num), None if r is None else r.ctypes.data,
                                   None if t is None else t.ctypes.data, cr.ctypes.data, cn.ctypes.data,
                                   len(commitments), out.ctypes.data)
    if rc:
        raise QpError(rc, lib().qp_ballot_box_last_error(None).decode())
    o = out[0]
    none = lambda v: None if int(v) == NOT_FOUND else int(v)  # noqa: E731
    return AuditReport(int(o["status"]), none(o["witness"]), none(o["first"]), [int(x) for x in o["root"]],
                       int(o["yes"]), int(o["no"]), int(o["counted"]))


class BallotBox(NullifierSetMixin):
    _SET_ABI = "qp_ballot_box"  # commit_nullifiers, nullifier_proofs, nullifier_proof_for, check_nullifier_proof

    def __init__(self, ctx_or_device, proposal_id, roots, verifier=None, capacity=None):
        """proposal_id: 4 canonical felts.  roots: the accepted Merkle roots, 1 to 64
        digests (a registry's `root` of every epoch ballots may refer to).  verifier:
        a WormholeVerifier of the voting circuit's data, needed by `cast` only.
        capacity: admitted ballots the box has room for (default 1024; `cast` grows
        it).  ctx_or_device: a Context, a device number (an own Context), or None
        for the host path."""
        prop = _digest(proposal_id, "proposal_id")
        roots = list(roots)
        if not 1 <= len(roots) <= MAX_ROOTS:
            raise ValueError(f"{len(roots)} accepted roots: a ballot box needs 1 to {MAX_ROOTS}")
        r = np.concatenate([_digest(x, "a root") for x in roots])
        capacity = DEFAULT_CAPACITY if capacity is None else int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError(f"capacity {capacity}: it must be 1 to 2^31 admitted ballots")
        self.verifier = verifier
        self.h = self._own_ctx = None
        if ctx_or_device is None or isinstance(ctx_or_device, Context):
            self.ctx = ctx_or_device
        else:
            self.ctx = self._own_ctx = Context(int(ctx_or_device))
        h = ctypes.c_void_p()
        rc = lib().qp_ballot_box_new(None if self.ctx is None else self.ctx.h, prop, r, len(roots), capacity,
                                     ctypes.byref(h))
        if rc:
            raise QpError(rc, lib().qp_ballot_box_last_error(None).decode())
        self.h = h

    def _check(self, rc):
        if rc:
            raise QpError(rc, lib().qp_ballot_box_last_error(self.h).decode())

    # ---- state
    def _state(self):
        c, a, cap = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().qp_ballot_box_state(self.h, ctypes.byref(c), ctypes.byref(a), ctypes.byref(cap)))
        return c.value, a.value, cap.value

    @property
    def cast_count(self):
        """ballots cast so far, rejected ones included: the next ballot's number"""
        return self._state()[0]

    @property
    def admitted(self):
        """ballots that passed the screen: counted ones and double votes (the log's length)"""
        return self._state()[1]

    @property
    def capacity(self):
        return self._state()[2]

    @property
    def tally(self):
        """(yes, no) of the counted ballots"""
        y, n = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(lib().qp_ballot_box_tally(self.h, ctypes.byref(y), ctypes.byref(n)))
        return y.value, n.value

    def accept_root(self, root):
        """One more accepted root (a new epoch's); a root already accepted is held once."""
        self._check(lib().qp_ballot_box_accept_root(self.h, _digest(root, "a root")))

    def reserve(self, capacity):
        """Moves the box to a log and table for `capacity` >= admitted ballots."""
        self._check(lib().qp_ballot_box_reserve(self.h, int(capacity)))

    def _make_room(self, n):
        """room for n more admitted ballots: double the capacity, or what the batch needs"""
        _, adm, cap = self._state()
        if adm + n > cap:
            if adm + n > MAX_CAPACITY:
                raise ValueError(f"{adm} + {n} ballots are more than 2^31, the most a box holds")
            self.reserve(min(max(2 * cap, adm + n), MAX_CAPACITY))

    @staticmethod
    def _results(out, raw):
        if raw:
            return out
        return [BallotResult(int(r["status"]), int(r["verify_status"]), int(r["number"]), int(r["first"])) for r in out]

    # ---- casting
    def cast(self, proofs, reserve=True, raw=False):
        """Verifies the voting proofs (bytes or ProofWithPublicInputs) and casts them:
        one BallotResult each (raw=True: a RESULT_DTYPE array).  A batch the capacity
        may not hold first reserves double (or what the batch needs); with
        reserve=False it is refused, as qp_ballot_box_cast does."""
        if self.verifier is None or self.verifier.h is None:
            raise ValueError("cast needs the box's verifier=: a WormholeVerifier of the voting circuit's data")
        datas = [bytes(p) if isinstance(p, (bytes, bytearray, memoryview)) else p.to_bytes() for p in proofs]
        n = len(datas)
        if n and reserve:
            self._make_room(n)
        ptrs = (ctypes.c_char_p * max(n, 1))(*datas)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in datas])
        out = np.zeros(n, RESULT_DTYPE)
        self._check(lib().qp_ballot_box_cast(self.h, self.verifier.h, ptrs, lens, n, out.ctypes.data))
        return self._results(out, raw)

    def cast_public(self, pis, verdicts=None, reserve=True, raw=False):
        """Casts ballots whose proofs were verified elsewhere, by their public inputs:
        pis [n][13] (a uint64 array, or rows of ints), verdicts [n] (non-zero marks a
        rejected proof; None: all verified).  A row that does not hold 13 values
        that fit 64 bits is cast as malformed."""
        if isinstance(pis, np.ndarray) and pis.dtype == np.uint64 and pis.ndim == 2 and pis.shape[1] == NPI:
            a = np.ascontiguousarray(pis)
        else:
            rows = [list(r) for r in pis]
            a = np.full((len(rows), NPI), np.uint64(2**64 - 1), np.uint64)  # not canonical: malformed
            for i, r in enumerate(rows):
                if len(r) == NPI and all(0 <= int(x) < 2**64 for x in r):
                    a[i] = [int(x) for x in r]
        n = a.shape[0]
        v = None
        if verdicts is not None:
            v = np.ascontiguousarray(verdicts, dtype=np.uint32)
            if v.shape != (n,):
                raise ValueError(f"{v.size} verdicts for {n} ballots")
        if n and reserve:
            self._make_room(n)
        out = np.zeros(n, RESULT_DTYPE)
        self._check(lib().qp_ballot_box_cast_public(self.h, a.ctypes.data, None if v is None else v.ctypes.data, n,
                                                    out.ctypes.data))
        return self._results(out, raw)

    # ---- publication and audit
    def entries(self, first=0, k=None):
        """The log, entries [first, first + k) in admission order (k=None: to the end):
        (nullifiers [k][4], numbers [k], counted [k] bool, votes [k] bool)."""
        first = int(first)
        k = max(self.admitted - first, 0) if k is None else int(k)
        nul = np.zeros((k, 4), np.uint64)
        num = np.zeros(k, np.uint64)
        fl = np.zeros(k, np.uint8)
        self._check(lib().qp_ballot_box_entries(self.h, first, k, nul.ctypes.data, num.ctypes.data, fl.ctypes.data))
        return nul, num, (fl & FLAG_COUNTED) != 0, (fl & FLAG_VOTE) != 0

    def recount(self):
        """(yes, no, counted, admitted) recomputed from the log's flags alone."""
        out = np.zeros(4, np.uint64)
        self._check(lib().qp_ballot_box_recount(self.h, out))
        return tuple(int(x) for x in out)

    # ---- the log commitment: what the operator publishes, and the voters' receipts
    def find(self, nullifiers, raw=False):
        """Per nullifier (4 canonical felts each; a [k][4] uint64 array, or rows of
        ints) the log index `seq` of its *counted* entry, or None if it was never
        admitted (raw=True: a uint64 array, NOT_FOUND for those).  A double vote's
        nullifier gives the counted entry, not the double's own."""
        if isinstance(nullifiers, np.ndarray) and nullifiers.dtype == np.uint64 and nullifiers.ndim == 2 \
                and nullifiers.shape[1] == 4:
            q = np.ascontiguousarray(nullifiers)
        else:
            rows = [[int(x) for x in n] for n in nullifiers]
            for i, r in enumerate(rows):
                if len(r) != 4 or any(not 0 <= x < 2**64 for x in r):
                    raise ValueError(f"nullifier at position {i} must be 4 field elements")
            q = np.array(rows, dtype=np.uint64).reshape(len(rows), 4)
        out = np.zeros(len(q), np.uint64)
        self._check(lib().qp_ballot_box_find(self.h, q.ctypes.data, len(q), out.ctypes.data))
        return out if raw else [None if int(s) == NOT_FOUND else int(s) for s in out]

    def commit_log(self):
        """(root, n): the commitment to log entries [0, n), n = admitted.  Brings the
        log tree up to date (only the new entries are hashed); refused on an empty log."""
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        self._check(lib().qp_ballot_box_commit_log(self.h, root.ctypes.data, ctypes.byref(n)))
        return [int(x) for x in root], n.value

    @property
    def log_root(self):
        return self.commit_log()[0]

    @property
    def log_size(self):
        return self.commit_log()[1]

    def roots_at(self, ms):
        """Per m in `ms` (each 1..admitted) the root the log had at m entries: the
        commitment (root, m) the box gave, or would have given, then.  Today's
        commitment extends an earlier one iff `roots_at([n_i]) == [root_i]`.
        Commits first, as `receipts` does."""
        m = np.array([int(x) for x in ms], dtype=np.uint64).reshape(-1)
        out = np.zeros((len(m), 4), np.uint64)
        self._check(lib().qp_ballot_box_roots_at(self.h, m.ctypes.data, len(m), out.ctypes.data))
        return [[int(x) for x in r] for r in out]

    def root_at(self, m):
        return self.roots_at([m])[0]

    @classmethod
    def restore(cls, ctx_or_device, proposal_id, roots, entries, cast_count=None, verifier=None, capacity=None,
                root=None):
        """Reopens a box from a published log (`entries`: what `entries()` returned, or
        (nullifiers, numbers, flags)) and continues from it: the arguments of the
        constructor, `cast_count` = the number the next ballot takes (None: the
        log's last number + 1), `capacity` (None: the default, or what the log
        needs), `root` = the log's published root, checked if given.  The log is
        audited first (canonical entries, increasing numbers, the count rule, the
        root); a log that fails raises QpError with the reason and the witness."""
        nul, num, fl = _log_arrays(entries)
        n = len(num)
        prop = _digest(proposal_id, "proposal_id")
        roots = list(roots)
        if not 1 <= len(roots) <= MAX_ROOTS:
            raise ValueError(f"{len(roots)} accepted roots: a ballot box needs 1 to {MAX_ROOTS}")
        r = np.concatenate([_digest(x, "a root") for x in roots])
        capacity = max(DEFAULT_CAPACITY, n) if capacity is None else int(capacity)
        if cast_count is None:
            cast_count = int(num[-1]) + 1 if n else 0
        expect = None if root is None else _digest(root, "root")
        self = cls.__new__(cls)
        self.verifier = verifier
        self.h = self._own_ctx = None
        if ctx_or_device is None or isinstance(ctx_or_device, Context):
            self.ctx = ctx_or_device
        else:
            self.ctx = self._own_ctx = Context(int(ctx_or_device))
        h = ctypes.c_void_p()
        rc = lib().qp_ballot_box_restore(None if self.ctx is None else self.ctx.h, prop, r, len(roots), capacity,
                                         nul.ctypes.data, num.ctypes.data, fl.ctypes.data, n, int(cast_count),
                                         None if expect is None else expect.ctypes.data, ctypes.byref(h))
        if rc:
            self.free()
            raise QpError(rc, lib().qp_ballot_box_last_error(None).decode())
        self.h = h
        return self

    def receipts(self, seqs):
        """One BallotReceipt per log index in `seqs`, all under one (root, n): the
        commitment after this call's own commit."""
        s = np.array([int(x) for x in seqs], dtype=np.uint64).reshape(-1)
        k = len(s)
        sib = np.zeros((k, PATH_SLOTS, 4), np.uint64)
        bits, depth = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        self._check(lib().qp_ballot_box_receipts(self.h, s.ctypes.data, k, sib.ctypes.data, bits.ctypes.data,
                                                 depth.ctypes.data, None, root.ctypes.data, ctypes.byref(n)))
        nul, num, fl = np.zeros((k, 4), np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint8)
        self._check(lib().qp_ballot_box_entries_at(self.h, s.ctypes.data, k, nul.ctypes.data, num.ctypes.data,
                                                   fl.ctypes.data))
        root = [int(x) for x in root]
        return [BallotReceipt([int(x) for x in nul[i]], int(num[i]), bool(fl[i] & FLAG_VOTE),
                              bool(fl[i] & FLAG_COUNTED), int(s[i]), sib[i, :depth[i]].tolist(), int(bits[i]),
                              int(depth[i]), root, n.value) for i in range(k)]

    def receipt_for(self, nullifier):
        """The receipt of the counted entry with this nullifier; None if it was never admitted."""
        seq = self.find([nullifier])[0]
        return None if seq is None else self.receipts([seq])[0]

    @staticmethod
    def check_receipt(r, root=None, n=None):
        """True iff receipt `r` holds under the published commitment (root, n), which
        default to the pair the receipt names.  A receipt is valid only under the
        (root, n) it was made under.  Needs no box and no device."""
        root = r.root if root is None else root
        n = r.n if n is None else n
        try:
            sib = np.zeros((PATH_SLOTS, 4), np.uint64)
            if r.siblings:
                sib[:len(r.siblings)] = np.array([[int(x) for x in d] for d in r.siblings], dtype=np.uint64)
            flags = (FLAG_VOTE if r.vote else 0) | (FLAG_COUNTED if r.counted else 0)
            rt = np.array([int(x) for x in root], dtype=np.uint64)
            nul = np.array([int(x) for x in r.nullifier], dtype=np.uint64)
            if rt.shape != (4,) or nul.shape != (4,):
                return False
            for v, bound in ((n, 2**64), (r.seq, 2**64), (r.number, 2**64), (r.path_bits, 2**32), (r.depth, 2**32)):
                if not 0 <= int(v) < bound:
                    return False
        except (OverflowError, ValueError, TypeError, IndexError):
            return False  # a value that fits no field of a receipt
        return lib().qp_ballot_receipt_check(rt.ctypes.data, int(n), int(r.seq), nul.ctypes.data, int(r.number), flags,
                                             sib.ctypes.data, int(r.path_bits), int(r.depth)) == 0

    def cast_times(self):
        """Device times of the last cast that admitted a ballot (ms): log upload, insert + resolve."""
        ms = (ctypes.c_double * 2)()
        self._check(lib().qp_ballot_box_cast_times(self.h, ms))
        return {"upload_ms": ms[0], "insert_resolve_ms": ms[1]}

    def free(self):
        if self.h:
            lib().qp_ballot_box_free(self.h)
            self.h = None
        if self._own_ctx is not None:
            self._own_ctx.close()
            self._own_ctx = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
