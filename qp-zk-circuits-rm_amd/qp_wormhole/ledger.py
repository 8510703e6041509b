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
"""
import ctypes
from collections import namedtuple

import numpy as np

from ._native import Context, QpError, lib

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


class WormholeLedger:
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
