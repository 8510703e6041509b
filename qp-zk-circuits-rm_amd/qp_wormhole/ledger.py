"""WormholeLedger: the settler's side of the Wormhole circuit (include/qpgpu.h qp_ledger_*).

A verified Wormhole proof says only that some unspent transfer of
`funding_amount` under storage root `root_hash` may be paid to `exit_account`,
with this `nullifier`.  A ledger is opened with the storage roots of the blocks
the settler knows; it verifies batches of proofs through a WormholeVerifier (or
takes the leaves of a verified aggregation root), screens their 16 public inputs
(nullifier[0:4] root_hash[4:8] funding_amount[8:12] exit_account[12:16]),
admits each nullifier once and credits the amounts to the exit accounts.  Every
transfer cast gets a number, its position in the stream of all transfers cast
into the ledger, and a status, the first check it fails (TRANSFER_STATUS_TEXT, in
the checks' order after "credited").  Of the transfers with one nullifier the
one with the lowest number is credited; the others are double spends whose
`first` names it.  Statuses, the log and the totals depend on the transfer
stream alone, not on how it is cut into batches.

`padding` names the public inputs of the aggregator's padding proof
(`WormholeLedger.padding_of(aggregator)`): an aggregated root carries them for
every empty leaf, they look like a real transfer, and a ledger that does not
know them pays the dummy.

With a Context (or a device number) the log, the nullifier and account tables
and the sums live on the device, and the screen runs there too
(csrc/ledger.hip); with None the same semantics run on the host.

The settler publishes (root, n, payouts): `commit_log` commits the log to a
Merkle root (the ballot box's kind of tree over a 14-felt leaf), `receipts`
ties single entries to it, `check_receipt` checks one without a ledger, and
`audit_ledger_log` checks a published log against the root, the totals, the
payouts and earlier commitments published beside it.

A settler pays per round, per commitment (root_k, n_k): `payouts_between(n_{k-1},
n_k)` is what round k pays, `ledger_log_payouts` the same from the published log
alone.  `WormholeLedger.restore` reopens a ledger from its published log, so a
settler whose process died counts on with the nullifier set it had.

In place of the payout list a settler can publish one root per round:
`commit_claims(m0, m1)` commits the round's per-account totals, sorted by
account, to a Merkle root; `claim_for` gives an account what it is owed with a
short proof, or a proof that it is owed nothing; `check_claim` checks one
without a ledger, and `ledger_log_claims_root` recomputes the commitment from
the published log alone (claims.py).
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._native import Context, QpError, lib
from .claims import TOTAL_LIMBS, ClaimLeaf, ClaimsCommitment, PayoutClaim, check_claim, limbs_total
from .nullifier_set import NullifierSetMixin

P = 0xFFFFFFFF00000001
NPI = 16
MAX_ROOTS = 4096
MAX_CAPACITY = 1 << 31
MAX_BATCH = 1 << 22  # transfers per qp_ledger_cast / qp_ledger_cast_public call
DEFAULT_CAPACITY = 1024

# qp_transfer_status
CREDITED, PROOF_REJECTED, MALFORMED, PADDING, BAD_AMOUNT, UNKNOWN_ROOT, DOUBLE_SPEND = range(7)
TRANSFER_STATUS_TEXT = ("credited", "proof rejected", "malformed public inputs", "padding proof", "bad amount",
                        "unknown root", "double spend")
FLAG_CREDITED = 1

NOT_FOUND = 2**64 - 1  # qp_ledger_find: the nullifier was never admitted

TransferResult = namedtuple("TransferResult", "status verify_status number first")
# qp_transfer_result
RESULT_DTYPE = np.dtype([("status", np.uint32), ("verify_status", np.uint32), ("number", np.uint64),
                         ("first", np.uint64)])


# one log entry tied to a published commitment (root, n): amount is the four 32-bit limbs, most
# significant first (`total` puts them together); siblings are the `depth` digests of the levels where
# the entry's node was hashed, from the leaf up; path_bits bit j = side of sibling j
class TransferReceipt(namedtuple("TransferReceipt",
                                 "nullifier number amount account credited seq siblings path_bits depth root n")):
    __slots__ = ()

    @property
    def total(self):
        """the entry's amount as one exact int"""
        return _total(self.amount)


# qp_ledger_audit_status: the first reason that fires, in this order
(LEDGER_AUDIT_OK, LEDGER_AUDIT_NON_CANONICAL, LEDGER_AUDIT_ORDER, LEDGER_AUDIT_CREDIT_RULE, LEDGER_AUDIT_TOTALS,
 LEDGER_AUDIT_PAYOUTS, LEDGER_AUDIT_ROOT, LEDGER_AUDIT_COMMITMENT) = range(8)
LEDGER_AUDIT_STATUS_TEXT = ("ok", "non-canonical entry", "transfer numbers out of order", "credit rule broken",
                            "claimed totals differ", "claimed payouts differ", "claimed root differs",
                            "earlier commitment does not hold")
# the verdict on a published log: witness = the lowest offender (an entry's seq; for the payouts and
# the commitments an index into the claim), first = the lowest seq holding the witness's nullifier
# (credit rule only), None where there is none; root, credited, the exact total and the account count
# recomputed from the log (zero on a non-canonical one)
LedgerAuditReport = namedtuple("LedgerAuditReport", "status witness first root credited total accounts")
# qp_ledger_audit_report
LEDGER_AUDIT_DTYPE = np.dtype([("status", np.uint32), ("pad", np.uint32), ("witness", np.uint64), ("first", np.uint64),
                               ("root", np.uint64, 4), ("credited", np.uint64), ("sums", np.uint64, 4),
                               ("accounts", np.uint64)])
PATH_SLOTS = 32  # sibling slots of a receipt's path: the log tree is the registry's kind of tree


def _felts(v, n, what):
    d = [int(x) for x in v]
    if len(d) != n or any(not 0 <= x < P for x in d):
        raise ValueError(f"{what} must be {n} canonical field elements")
    return np.array(d, dtype=np.uint64)


def _account_felts(a):
    """an exit account as 4 felts: 32 bytes (the reference's BytesDigest, little-endian words) or 4 ints"""
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = bytes(a)
        if len(a) != 32:
            raise ValueError("an account is 32 bytes or 4 field elements")
        return [int.from_bytes(a[i:i + 8], "little") for i in range(0, 32, 8)]
    return [int(x) for x in a]


def _total(sums):
    """the exact total of four limb sums, most significant first"""
    return sum(int(s) << (96 - 32 * i) for i, s in enumerate(sums))


def _keys(rows, what):
    if isinstance(rows, np.ndarray) and rows.dtype == np.uint64 and rows.ndim == 2 and rows.shape[1] == 4:
        return np.ascontiguousarray(rows)
    rows = [_account_felts(r) for r in rows]
    for i, r in enumerate(rows):
        if len(r) != 4 or any(not 0 <= x < 2**64 for x in r):
            raise ValueError(f"{what} at position {i} must be 4 field elements")
    return np.array(rows, dtype=np.uint64).reshape(len(rows), 4)


def _limbs(amounts, n):
    """amounts as [n][4] uint32 limbs: that array itself, or exact ints split most significant limb first"""
    if isinstance(amounts, np.ndarray) and amounts.ndim == 2:
        if amounts.shape != (n, 4):
            raise ValueError(f"amount limbs of shape {amounts.shape} for {n} entries")
        return np.ascontiguousarray(amounts, dtype=np.uint32)
    ints = [int(a) for a in amounts]
    if len(ints) != n or any(not 0 <= a < 1 << 128 for a in ints):
        raise ValueError(f"amounts must be {n} ints below 2^128, or [{n}][4] limbs")
    return np.array([[(a >> (96 - 32 * i)) & 0xFFFFFFFF for i in range(4)] for a in ints], dtype=np.uint32).reshape(n, 4)


def _sum_words(v):
    """four words that name a total (sum of words[i] << (96 - 32 i)): limb sums as they are, or an
    exact int split with the top word taking what is above 2^96"""
    if isinstance(v, (int, np.integer)):
        t = int(v)
        if not 0 <= t < 1 << 160:
            raise ValueError("a total is an int in [0, 2^160)")
        return [t >> 96, (t >> 64) & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF, t & 0xFFFFFFFF]
    w = [int(x) for x in v]
    if len(w) != 4 or any(not 0 <= x < 2**64 for x in w):
        raise ValueError("limb sums are four values that fit 64 bits")
    return w


def _ledger_log_arrays(entries):
    """(nullifiers [n][4], numbers [n], amounts [n][4] u32, accounts [n][4], flags [n] u8) of a published
    log: the 5-tuple `WormholeLedger.entries()` returns (exact-int amounts, credited bools), or the same
    with [n][4] limbs and/or a uint8 flags array"""
    entries = tuple(entries)
    if len(entries) != 5:
        raise ValueError("a log is (nullifiers, numbers, amounts, accounts, credited or flags)")
    nul, num, amt, acc, fl = entries
    nul = np.ascontiguousarray(nul, dtype=np.uint64).reshape(-1, 4)
    num = np.ascontiguousarray(num, dtype=np.uint64).reshape(-1)
    acc = np.ascontiguousarray(acc, dtype=np.uint64).reshape(-1, 4)
    fl = np.asarray(fl)
    fl = fl.astype(np.uint8) * FLAG_CREDITED if fl.dtype == bool else fl.astype(np.uint8)
    fl = np.ascontiguousarray(fl).reshape(-1)
    n = len(num)
    amt = _limbs(amt, n)
    if not len(nul) == len(acc) == len(fl) == n:
        raise ValueError(f"a log of {len(nul)} nullifiers, {n} numbers, {len(acc)} accounts and {len(fl)} flags")
    return nul, num, amt, acc, fl


def audit_ledger_log(ctx_or_none, entries, root=None, totals=None, payouts=None, commitments=()):
    """Audits a published transfer log (`entries`: what `WormholeLedger.entries()`
    returned) against what was published beside it, each optional: `root` (4
    felts); `totals` = (credited, total) with the total an exact int or four limb
    sums; `payouts` as `WormholeLedger.payouts()` returned them, either form;
    earlier `commitments` [(root_i, n_i), ...].  Returns a LedgerAuditReport whose
    status is the first reason that fires (LEDGER_AUDIT_STATUS_TEXT), with the
    lowest offender as the witness.  With a Context the audit runs on the device
    (csrc/ledger.hip), with None on the host; it needs no ledger and does not alter
    the log."""
    nul, num, amt, acc, fl = _ledger_log_arrays(entries)
    r = None if root is None else np.array([int(x) for x in root], dtype=np.uint64)
    if r is not None and r.shape != (4,):
        raise ValueError("root is 4 field elements")
    t = None
    if totals is not None:
        credited, total = totals
        t = np.array([int(credited)] + _sum_words(total), dtype=np.uint64)
    pa = ps = pf = None
    npay = 0
    if payouts is not None:
        if isinstance(payouts, tuple) and len(payouts) == 3 and isinstance(payouts[0], np.ndarray):
            # the raw form: accounts [k][4], limb sums [k][4], first_seq [k], taken as the arrays they are
            a, s, f = (np.asarray(x) for x in payouts)
            npay = len(f)
            if not (a.shape == s.shape == (npay, 4) and f.shape == (npay,)
                    and a.dtype == s.dtype == f.dtype == np.uint64):
                raise ValueError("raw payouts are uint64 arrays (accounts [k][4], sums [k][4], first_seq [k])")
            pa, ps, pf = (np.ascontiguousarray(x) if npay else np.zeros_like(x, shape=(1,) + x.shape[1:])
                          for x in (a, s, f))
        else:
            rows = list(payouts)
            npay = len(rows)
            pa = np.zeros((max(npay, 1), 4), np.uint64)
            ps = np.zeros((max(npay, 1), 4), np.uint64)
            pf = np.zeros(max(npay, 1), np.uint64)
            for i, (a, s, f) in enumerate(rows):
                pa[i], ps[i], pf[i] = _account_felts(a), _sum_words(s), int(f)
    commitments = list(commitments)
    cr = np.array([[int(x) for x in c[0]] for c in commitments], dtype=np.uint64).reshape(len(commitments), 4)
    cn = np.array([int(c[1]) for c in commitments], dtype=np.uint64)
    out = np.zeros(1, LEDGER_AUDIT_DTYPE)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib().qp_ledger_log_audit(None if ctx_or_none is None else ctx_or_none.h, nul.ctypes.data, num.ctypes.data,
                                   amt.ctypes.data, acc.ctypes.data, fl.ctypes.data, len(num), ptr(r), ptr(t), ptr(pa),
                                   ptr(ps), ptr(pf), npay, cr.ctypes.data, cn.ctypes.data, len(commitments),
                                   out.ctypes.data)
    if rc:
        raise QpError(rc, lib().qp_ledger_last_error(None).decode())
    o = out[0]
    none = lambda v: None if int(v) == NOT_FOUND else int(v)  # noqa: E731
    return LedgerAuditReport(int(o["status"]), none(o["witness"]), none(o["first"]), [int(x) for x in o["root"]],
                             int(o["credited"]), _total(o["sums"]), int(o["accounts"]))


def _round_rows(call, m0, m1, raw):
    """the rows of a payout round in one call (a range has at most m1 - m0 accounts, so no sizing call,
    which would run the round twice); call(cap, accounts, sums, first_seq, count) raises on a refusal"""
    room = max(m1 - m0, 0) if m1 <= MAX_CAPACITY else 0  # a range the call refuses: no buffers
    acc, sums, seq = np.zeros((room, 4), np.uint64), np.zeros((room, 4), np.uint64), np.zeros(room, np.uint64)
    count = ctypes.c_uint64()
    call(room, acc.ctypes.data, sums.ctypes.data, seq.ctypes.data, ctypes.byref(count))
    k = count.value
    acc, sums, seq = acc[:k].copy(), sums[:k].copy(), seq[:k].copy()
    if raw:
        return acc, sums, seq
    return [(acc[i].astype("<u8").tobytes(), _total(sums[i]), int(seq[i])) for i in range(k)]


def ledger_log_payouts(ctx_or_none, entries, m0=0, m1=None, raw=False):
    """What the round [m0, m1) of a published transfer log pays (`entries`: what
    `WormholeLedger.entries()` returned; m1=None: to the end), as
    `WormholeLedger.payouts_between` gives it: [(account 32 bytes, exact total,
    first_seq)] over the credited entries of the range, in first_seq order.  An
    auditor compares it with the list the settler published for the commitment
    (root_k, n_k), m0 = n_{k-1}, m1 = n_k.  The flags are trusted: `audit_ledger_log`
    is what checks them.  With a Context the range alone is uploaded and credited on
    the device, with None on the host; needs no ledger."""
    _, _, amt, acc, fl = _ledger_log_arrays(entries)
    n = len(fl)
    m0, m1 = int(m0), n if m1 is None else int(m1)

    def call(cap, a, s, f, count):
        rc = lib().qp_ledger_log_payouts_between(None if ctx_or_none is None else ctx_or_none.h, acc.ctypes.data,
                                                 amt.ctypes.data, fl.ctypes.data, n, m0, m1, cap, a, s, f, count)
        if rc:
            raise QpError(rc, lib().qp_ledger_last_error(None).decode())
    return _round_rows(call, m0, m1, raw)


def ledger_log_claims_root(ctx_or_none, entries, m0=0, m1=None):
    """(root, count, total, order): the payout claims commitment of round [m0, m1) of a
    published transfer log (`entries`: what `WormholeLedger.entries()` returned;
    m1=None: to the end), as `WormholeLedger.commit_claims` gives it, and the rows'
    first_seq in sorted order.  An auditor compares (root, count, total) with what
    the settler published for the round.  The flags are trusted: `audit_ledger_log`
    is what checks them.  With a Context the range alone is uploaded and committed
    on the device, with None on the host; needs no ledger."""
    _, _, amt, acc, fl = _ledger_log_arrays(entries)
    n = len(fl)
    m0, m1 = int(m0), n if m1 is None else int(m1)
    room = max(m1 - m0, 0) if m1 <= MAX_CAPACITY else 0  # a range the call refuses: no buffer
    root, count, total = np.zeros(4, np.uint64), ctypes.c_uint64(), np.zeros(TOTAL_LIMBS, np.uint32)
    order = np.zeros(max(room, 1), np.uint64)
    rc = lib().qp_ledger_log_claims_root(None if ctx_or_none is None else ctx_or_none.h, acc.ctypes.data, amt.ctypes.data,
                                         fl.ctypes.data, n, m0, m1, root.ctypes.data, ctypes.byref(count),
                                         total.ctypes.data, order.ctypes.data)
    if rc:
        raise QpError(rc, lib().qp_ledger_last_error(None).decode())
    return [int(x) for x in root], count.value, limbs_total(total), [int(x) for x in order[:count.value]]


class WormholeLedger(NullifierSetMixin):
    _SET_ABI = "qp_ledger"  # commit_nullifiers, nullifier_proofs, nullifier_proof_for, check_nullifier_proof

    def __init__(self, ctx_or_device, roots, padding=None, verifier=None, capacity=None):
        """roots: the accepted storage roots, 1 to 4096 digests of 4 canonical felts.
        padding: the 16 public inputs of the aggregator's padding proof
        (`padding_of`), or None.  verifier: a WormholeVerifier of the Wormhole
        circuit's data, needed by `cast` only.  capacity: admitted transfers the
        ledger has room for (default 1024; the cast methods grow it).
        ctx_or_device: a Context, a device number (an own Context), or None for
        the host path."""
        roots = list(roots)
        if not 1 <= len(roots) <= MAX_ROOTS:
            raise ValueError(f"{len(roots)} accepted roots: a ledger needs 1 to {MAX_ROOTS}")
        r = np.concatenate([_felts(x, 4, "a root") for x in roots])
        pad = None if padding is None else _felts(padding, NPI, "padding")
        capacity = DEFAULT_CAPACITY if capacity is None else int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError(f"capacity {capacity}: it must be 1 to 2^31 admitted transfers")
        self.verifier = verifier
        self.h = self._own_ctx = None
        if ctx_or_device is None or isinstance(ctx_or_device, Context):
            self.ctx = ctx_or_device
        else:
            self.ctx = self._own_ctx = Context(int(ctx_or_device))
        h = ctypes.c_void_p()
        rc = lib().qp_ledger_new(None if self.ctx is None else self.ctx.h, r.ctypes.data, len(roots),
                                 None if pad is None else pad.ctypes.data, capacity, ctypes.byref(h))
        if rc:
            raise QpError(rc, lib().qp_ledger_last_error(None).decode())
        self.h = h

    @classmethod
    def restore(cls, ctx_or_none, roots, entries, cast_count=None, padding=None, verifier=None, capacity=None,
                root=None):
        """Reopens a ledger from its published log (`entries`: what `entries()`
        returned) and continues from it: the arguments of the constructor,
        `cast_count` = the number the next transfer takes (None: the log's last
        number + 1, 0 for an empty log), `capacity` (None: the default, or what the
        log needs), `root` = the log's published root, checked if given.  The log is
        audited first (canonical entries, increasing numbers, the credit rule, the
        root); a log that fails raises ValueError with the reason
        (LEDGER_AUDIT_STATUS_TEXT) and the witness.  The restored ledger has the
        nullifier set, the account totals and the log of the ledger that published
        it: a repeat of an old transfer is a double spend naming the original."""
        nul, num, amt, acc, fl = _ledger_log_arrays(entries)
        n = len(num)
        roots = list(roots)
        if not 1 <= len(roots) <= MAX_ROOTS:
            raise ValueError(f"{len(roots)} accepted roots: a ledger needs 1 to {MAX_ROOTS}")
        r = np.concatenate([_felts(x, 4, "a root") for x in roots])
        pad = None if padding is None else _felts(padding, NPI, "padding")
        capacity = max(DEFAULT_CAPACITY, n) if capacity is None else int(capacity)
        if cast_count is None:
            cast_count = int(num[-1]) + 1 if n else 0
        expect = None if root is None else _felts(root, 4, "root")
        self = cls.__new__(cls)
        self.verifier = verifier
        self.h = self._own_ctx = None
        if ctx_or_none is None or isinstance(ctx_or_none, Context):
            self.ctx = ctx_or_none
        else:
            self.ctx = self._own_ctx = Context(int(ctx_or_none))
        h = ctypes.c_void_p()
        rc = lib().qp_ledger_restore(None if self.ctx is None else self.ctx.h, r.ctypes.data, len(roots),
                                     None if pad is None else pad.ctypes.data, capacity, nul.ctypes.data,
                                     num.ctypes.data, amt.ctypes.data, acc.ctypes.data, fl.ctypes.data, n,
                                     int(cast_count), None if expect is None else expect.ctypes.data, ctypes.byref(h))
        if rc:
            why = lib().qp_ledger_last_error(None).decode()
            self.free()
            if rc == 6:  # QP_ERR_FORMAT: the log fails its audit
                raise ValueError(why)
            raise QpError(rc, why)
        self.h = h
        return self

    @staticmethod
    def padding_of(aggregator):
        """The 16 public inputs of `aggregator.dummy_proof()`: what an aggregated
        root carries for every leaf the aggregator padded."""
        return [int(x) for x in aggregator.dummy_proof().public_inputs]

    def _check(self, rc):
        if rc:
            raise QpError(rc, lib().qp_ledger_last_error(self.h).decode())

    # ---- state
    def _state(self):
        v = [ctypes.c_uint64() for _ in range(5)]
        self._check(lib().qp_ledger_state(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @property
    def cast_count(self):
        """transfers cast so far, rejected ones included: the next transfer's number"""
        return self._state()[0]

    @property
    def admitted(self):
        """transfers that passed the screen: credited ones and double spends (the log's length)"""
        return self._state()[1]

    @property
    def credited(self):
        return self._state()[2]

    @property
    def accounts(self):
        """exit accounts credited so far"""
        return self._state()[3]

    @property
    def capacity(self):
        return self._state()[4]

    def accept_root(self, root):
        """One more accepted root (a new block's); a root already accepted is held once."""
        self._check(lib().qp_ledger_accept_root(self.h, _felts(root, 4, "a root").ctypes.data))

    def reserve(self, capacity):
        """Moves the ledger to a log and tables for `capacity` >= admitted transfers."""
        self._check(lib().qp_ledger_reserve(self.h, int(capacity)))

    def _make_room(self, n):
        """room for n more admitted transfers: double the capacity, or what the batch needs"""
        _, adm, _, _, cap = self._state()
        if adm + n > cap:
            if adm + n > MAX_CAPACITY:
                raise ValueError(f"{adm} + {n} transfers are more than 2^31, the most a ledger holds")
            self.reserve(min(max(2 * cap, adm + n), MAX_CAPACITY))

    @staticmethod
    def _results(out, raw):
        if raw:
            return out
        return [TransferResult(int(r["status"]), int(r["verify_status"]), int(r["number"]), int(r["first"]))
                for r in out]

    # ---- casting
    def cast(self, proofs, reserve=True, raw=False):
        """Verifies the Wormhole proofs (bytes or ProofWithPublicInputs) and casts
        them: one TransferResult each (raw=True: a RESULT_DTYPE array).  A batch the
        capacity may not hold first reserves double (or what the batch needs); with
        reserve=False it is refused, as qp_ledger_cast does."""
        if self.verifier is None or self.verifier.h is None:
            raise ValueError("cast needs the ledger's verifier=: a WormholeVerifier of the Wormhole circuit's data")
        datas = [bytes(p) if isinstance(p, (bytes, bytearray, memoryview)) else p.to_bytes() for p in proofs]
        out = np.zeros(len(datas), RESULT_DTYPE)
        for at in range(0, len(datas), MAX_BATCH):
            part = datas[at:at + MAX_BATCH]
            n = len(part)
            if reserve:
                self._make_room(n)
            ptrs = (ctypes.c_char_p * n)(*part)
            lens = (ctypes.c_size_t * n)(*[len(d) for d in part])
            self._check(lib().qp_ledger_cast(self.h, self.verifier.h, ptrs, lens, n, out[at:].ctypes.data))
        return self._results(out, raw)

    def cast_public(self, pis, verdicts=None, reserve=True, raw=False):
        """Casts transfers whose proofs were verified elsewhere, by their public
        inputs: pis [n][16] (a uint64 array, or rows of ints), verdicts [n]
        (non-zero marks a rejected proof; None: all verified).  A row that does not
        hold 16 values that fit 64 bits is cast as malformed.  More than 2^22
        transfers go in as several calls."""
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
                raise ValueError(f"{v.size} verdicts for {n} transfers")
        out = np.zeros(n, RESULT_DTYPE)
        for at in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - at)
            if reserve:
                self._make_room(m)
            self._check(lib().qp_ledger_cast_public(self.h, a[at:].ctypes.data, None if v is None else v[at:].ctypes.data,
                                                    m, out[at:].ctypes.data))
        return self._results(out, raw)

    def cast_aggregated(self, aggregator, root_proof, reserve=True, raw=False):
        """Verifies an aggregated root (an AggregatedProof of `aggregator`, a
        WormholeProofAggregator) with its aggregation circuit's verifier data and
        casts the leaves `aggregator.extract_leaf_public_inputs` reads out of it,
        padding leaves included.  If the root fails verification every leaf is
        cast as a rejected proof, with the root's verdict."""
        from .verifier import WormholeVerifier
        proof, cd = root_proof.proof, root_proof.circuit_data
        pis = [int(x) for x in proof.public_inputs]
        leaves = aggregator.config.num_leaf_proofs
        if len(pis) != NPI * leaves:
            raise ValueError(f"aggregated public inputs should contain: {NPI * leaves} (= {leaves} leaves x {NPI} "
                             f"fields), got: {len(pis)}")
        ver = WormholeVerifier(circuit_data=(cd.verifier_only, cd.common),
                               device=None if self.ctx is None else aggregator.device, max_batch=1)
        try:
            verdict = ver.verify_batch([proof])[0]
        finally:
            ver.close()
        rows = np.array(pis, dtype=np.uint64).reshape(leaves, NPI)
        return self.cast_public(rows, None if verdict == 0 else [verdict] * leaves, reserve=reserve, raw=raw)

    # ---- lookups, publication and audit
    def find(self, nullifiers, raw=False):
        """Per nullifier (4 canonical felts each; a [k][4] uint64 array, or rows of
        ints) the log index of its credited entry, or None if it was never admitted
        (raw=True: a uint64 array, NOT_FOUND for those)."""
        q = _keys(nullifiers, "nullifier")
        out = np.zeros(len(q), np.uint64)
        self._check(lib().qp_ledger_find(self.h, q.ctypes.data, len(q), out.ctypes.data))
        return out if raw else [None if int(s) == NOT_FOUND else int(s) for s in out]

    def entries(self, first=0, k=None):
        """The log, entries [first, first + k) in admission order (k=None: to the end):
        (nullifiers [k][4], numbers [k], amounts [k] exact ints, accounts [k][4],
        credited [k] bool)."""
        first = int(first)
        k = max(self.admitted - first, 0) if k is None else int(k)
        nul, acc = np.zeros((k, 4), np.uint64), np.zeros((k, 4), np.uint64)
        num, amt, fl = np.zeros(k, np.uint64), np.zeros((k, 4), np.uint32), np.zeros(k, np.uint8)
        self._check(lib().qp_ledger_entries(self.h, first, k, nul.ctypes.data, num.ctypes.data, amt.ctypes.data,
                                            acc.ctypes.data, fl.ctypes.data))
        return nul, num, [_total(a) for a in amt], acc, (fl & FLAG_CREDITED) != 0

    def payouts(self, raw=False):
        """[(account 32 bytes, exact total, first_seq)] for every account credited so
        far, in the order of the log index of each account's first credited entry
        (raw=True: the arrays accounts [k][4], limb sums [k][4], first_seq [k])."""
        k = self.accounts
        acc, sums, seq = np.zeros((k, 4), np.uint64), np.zeros((k, 4), np.uint64), np.zeros(k, np.uint64)
        self._check(lib().qp_ledger_payouts(self.h, 0, k, acc.ctypes.data, sums.ctypes.data, seq.ctypes.data))
        if raw:
            return acc, sums, seq
        return [(acc[i].astype("<u8").tobytes(), _total(sums[i]), int(seq[i])) for i in range(k)]

    def payouts_between(self, m0, m1, raw=False):
        """What the round of log entries [m0, m1) pays (0 <= m0 <= m1 <= admitted):
        [(account 32 bytes, exact total, first_seq)] over the credited entries of
        the range alone, in first_seq order; an account credited before m0 and again
        inside appears with its in-range total and first_seq (raw=True: the arrays
        accounts [k][4], limb sums [k][4], first_seq [k]).  A settler publishes
        (root_k, n_k, payouts_between(n_{k-1}, n_k)) per commitment; the rounds add
        up to `payouts()`.  The ledger is not changed."""
        m0, m1 = int(m0), int(m1)

        def call(cap, a, s, f, count):
            self._check(lib().qp_ledger_payouts_between(self.h, m0, m1, cap, a, s, f, count))
        return _round_rows(call, m0, m1, raw)

    # ---- payout claims: one root per round, a short proof per payee (claims.py has the definitions)
    def _claims_range(self, m0, m1):
        return int(m0), self.admitted if m1 is None else int(m1)

    def commit_claims(self, m0=0, m1=None):
        """ClaimsCommitment(root, count, total, m0, m1) of the round of log entries
        [m0, m1) (m1=None: to the end): the root over the rows of
        `payouts_between(m0, m1)` sorted by account, their number, and the exact sum
        of their totals.  A settler publishes it in place of the payout list.  The
        ledger keeps one range's tree: the same range again does no work."""
        m0, m1 = self._claims_range(m0, m1)
        root, count, total = np.zeros(4, np.uint64), ctypes.c_uint64(), np.zeros(TOTAL_LIMBS, np.uint32)
        self._check(lib().qp_ledger_commit_claims(self.h, m0, m1, root.ctypes.data, ctypes.byref(count),
                                                  total.ctypes.data))
        return ClaimsCommitment([int(x) for x in root], count.value, limbs_total(total), m0, m1)

    def claims(self, accounts, m0=0, m1=None):
        """One PayoutClaim per account (32 bytes or 4 canonical felts), all under the
        commitment of round [m0, m1): what the account is owed with its path, or the
        two adjacent leaves that show it is owed nothing."""
        m0, m1 = self._claims_range(m0, m1)
        q = _keys(accounts, "account")
        k = len(q)
        found, pos = np.zeros(k, np.uint8), np.zeros(k, np.uint64)
        acc = [np.zeros((k, 4), np.uint64) for _ in range(2)]
        tot = [np.zeros((k, TOTAL_LIMBS), np.uint32) for _ in range(2)]
        seq = [np.zeros(k, np.uint64) for _ in range(2)]
        sib = [np.zeros((k, PATH_SLOTS, 4), np.uint64) for _ in range(2)]
        bits = [np.zeros(k, np.uint32) for _ in range(2)]
        depth = [np.zeros(k, np.uint32) for _ in range(2)]
        root, count = np.zeros(4, np.uint64), ctypes.c_uint64()
        args = [self.h, m0, m1, q.ctypes.data, k, found.ctypes.data, pos.ctypes.data]
        for s in range(2):
            args += [acc[s].ctypes.data, tot[s].ctypes.data, seq[s].ctypes.data, sib[s].ctypes.data, bits[s].ctypes.data,
                     depth[s].ctypes.data]
        self._check(lib().qp_ledger_claims(*args, root.ctypes.data, ctypes.byref(count)))
        root, count = [int(x) for x in root], count.value

        def leaf(s, i):
            return ClaimLeaf([int(x) for x in acc[s][i]], limbs_total(tot[s][i]), int(seq[s][i]),
                             sib[s][i, :depth[s][i]].tolist(), int(bits[s][i]), int(depth[s][i]))

        out = []
        for i in range(k):
            f, p = bool(found[i]), int(pos[i])
            out.append(PayoutClaim([int(x) for x in q[i]], f, p, leaf(0, i) if not f and p > 0 else None,
                                   leaf(1, i) if p < count else None, root, count, m0, m1))
        return out

    def claim_for(self, account, m0=0, m1=None):
        return self.claims([account], m0, m1)[0]

    check_claim = staticmethod(check_claim)

    def totals_for(self, accounts):
        """Per account (32 bytes or 4 felts) its exact total, or None if it was never credited."""
        q = _keys(accounts, "account")
        sums, found = np.zeros((len(q), 4), np.uint64), np.zeros(len(q), np.uint8)
        self._check(lib().qp_ledger_totals_for(self.h, q.ctypes.data, len(q), sums.ctypes.data, found.ctypes.data))
        return [_total(sums[i]) if found[i] else None for i in range(len(q))]

    def total_for(self, account):
        """The exact total credited to `account` so far (0 if it was never credited)."""
        return self.totals_for([account])[0] or 0

    def recount(self):
        """(credited, admitted, total) recomputed from the log alone; total is the
        exact sum of every credited amount and equals the sum of the payouts."""
        out = np.zeros(6, np.uint64)
        self._check(lib().qp_ledger_recount(self.h, out.ctypes.data))
        return int(out[0]), int(out[1]), _total(out[2:])

    # ---- the log commitment: what the settler publishes, and the exit accounts' receipts
    def commit_log(self):
        """(root, n): the commitment to log entries [0, n), n = admitted.  Brings the
        log tree up to date (only the new entries are hashed); refused on an empty
        log.  The settler publishes (root, n, payouts)."""
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        self._check(lib().qp_ledger_commit_log(self.h, root.ctypes.data, ctypes.byref(n)))
        return [int(x) for x in root], n.value

    @property
    def log_root(self):
        return self.commit_log()[0]

    @property
    def log_size(self):
        return self.commit_log()[1]

    def roots_at(self, ms):
        """Per m in `ms` (each 1..admitted) the root the log had at m entries: the
        commitment (root, m) the ledger gave, or would have given, then.  Commits
        first, as `receipts` does."""
        m = np.array([int(x) for x in ms], dtype=np.uint64).reshape(-1)
        out = np.zeros((len(m), 4), np.uint64)
        self._check(lib().qp_ledger_roots_at(self.h, m.ctypes.data, len(m), out.ctypes.data))
        return [[int(x) for x in r] for r in out]

    def root_at(self, m):
        return self.roots_at([m])[0]

    def entries_at(self, seqs):
        """The log entries at the indices `seqs` (any order), as `entries` gives them:
        (nullifiers [k][4], numbers [k], amounts [k] exact ints, accounts [k][4],
        credited [k] bool)."""
        nul, num, amt, acc, fl = self._entries_at(np.array([int(x) for x in seqs], dtype=np.uint64).reshape(-1))
        return nul, num, [_total(a) for a in amt], acc, (fl & FLAG_CREDITED) != 0

    def _entries_at(self, s):
        k = len(s)
        nul, acc = np.zeros((k, 4), np.uint64), np.zeros((k, 4), np.uint64)
        num, amt, fl = np.zeros(k, np.uint64), np.zeros((k, 4), np.uint32), np.zeros(k, np.uint8)
        self._check(lib().qp_ledger_entries_at(self.h, s.ctypes.data, k, nul.ctypes.data, num.ctypes.data,
                                               amt.ctypes.data, acc.ctypes.data, fl.ctypes.data))
        return nul, num, amt, acc, fl

    def receipts(self, seqs):
        """One TransferReceipt per log index in `seqs`, all under one (root, n): the
        commitment after this call's own commit."""
        s = np.array([int(x) for x in seqs], dtype=np.uint64).reshape(-1)
        k = len(s)
        sib = np.zeros((k, PATH_SLOTS, 4), np.uint64)
        bits, depth = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        self._check(lib().qp_ledger_receipts(self.h, s.ctypes.data, k, sib.ctypes.data, bits.ctypes.data,
                                             depth.ctypes.data, None, root.ctypes.data, ctypes.byref(n)))
        nul, num, amt, acc, fl = self._entries_at(s)
        root = [int(x) for x in root]
        return [TransferReceipt([int(x) for x in nul[i]], int(num[i]), [int(x) for x in amt[i]],
                                [int(x) for x in acc[i]], bool(fl[i] & FLAG_CREDITED), int(s[i]),
                                sib[i, :depth[i]].tolist(), int(bits[i]), int(depth[i]), root, n.value)
                for i in range(k)]

    def receipt_for(self, nullifier):
        """The receipt of the credited entry with this nullifier; None if it was never admitted."""
        seq = self.find([nullifier])[0]
        return None if seq is None else self.receipts([seq])[0]

    @staticmethod
    def check_receipt(r, root=None, n=None):
        """True iff receipt `r` holds under the published commitment (root, n), which
        default to the pair the receipt names.  A receipt is valid only under the
        (root, n) it was made under.  Needs no ledger and no device."""
        root = r.root if root is None else root
        n = r.n if n is None else n
        try:
            sib = np.zeros((PATH_SLOTS, 4), np.uint64)
            if r.siblings:
                sib[:len(r.siblings)] = np.array([[int(x) for x in d] for d in r.siblings], dtype=np.uint64)
            rt = np.array([int(x) for x in root], dtype=np.uint64)
            nul = np.array([int(x) for x in r.nullifier], dtype=np.uint64)
            acc = np.array([int(x) for x in r.account], dtype=np.uint64)
            amt = np.array([int(x) for x in r.amount], dtype=np.uint64)
            if rt.shape != (4,) or nul.shape != (4,) or acc.shape != (4,) or amt.shape != (4,) or (amt >> 32).any():
                return False
            amt = amt.astype(np.uint32)
            for v, bound in ((n, 2**64), (r.seq, 2**64), (r.number, 2**64), (r.path_bits, 2**32), (r.depth, 2**32)):
                if not 0 <= int(v) < bound:
                    return False
        except (OverflowError, ValueError, TypeError, IndexError):
            return False  # a value that fits no field of a receipt
        return lib().qp_ledger_receipt_check(rt.ctypes.data, int(n), int(r.seq), nul.ctypes.data, int(r.number),
                                             amt.ctypes.data, acc.ctypes.data, 1 if r.credited else 0, sib.ctypes.data,
                                             int(r.path_bits), int(r.depth)) == 0

    def cast_times(self):
        """Device times of the last cast (ms): upload, screen to credit."""
        ms = (ctypes.c_double * 2)()
        self._check(lib().qp_ledger_cast_times(self.h, ms))
        return {"upload_ms": ms[0], "kernels_ms": ms[1]}

    def free(self):
        if self.h:
            lib().qp_ledger_free(self.h)
            self.h = None
        if self._own_ctx is not None:
            self._own_ctx.close()
            self._own_ctx = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
