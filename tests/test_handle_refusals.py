"""The refusals that qp_ballot_box_* and qp_ledger_* word alike
(csrc/handle_common.h, csrc/audit_common.h), on the host path (ctx NULL): the
return code and the exact *_last_error text of each, at capacity 8 with three
admitted entries.  The texts are literals; they were taken from the library as
it was before the two handles shared this code.  CASES is also run on the
device path by tests/test_gpu_handle_refusals.py."""
import ctypes

import numpy as np
import pytest

from ballot_model import P, PROPOSAL, ROOT_A, ballot
from ledger_model import transfer

ARG, STATE, FORMAT = 1, 4, 6
CAPACITY, ADMITTED = 8, 3
NULLIFIERS = [[7, 0, 0, i] for i in range(9)]


def u64(x):
    return np.ascontiguousarray(x, dtype=np.uint64)


class Box:
    """the calls of a ballot box that the table needs, by the names the ledger has for them"""
    abi, audit = "qp_ballot_box", "qp_ballot_log_audit"

    @staticmethod
    def open(ctx, capacity=CAPACITY):
        from qp_wormhole import BallotBox
        return BallotBox(ctx, PROPOSAL, [ROOT_A], capacity=capacity)

    @staticmethod
    def pis(nullifiers):
        return [ballot(q) for q in nullifiers]

    @staticmethod
    def restore(L, c, capacity, log, cast_count, root, out):
        nul, num, fl = log
        return L.qp_ballot_box_restore(c, u64(PROPOSAL), u64(ROOT_A), 1, capacity, nul.ctypes.data, num.ctypes.data,
                                       fl.ctypes.data, len(num), cast_count, root, out)

    @staticmethod
    def audit_commitment(L, c, log, roots, ns, report):
        nul, num, fl = log
        return L.qp_ballot_log_audit(c, nul.ctypes.data, num.ctypes.data, fl.ctypes.data, len(num), None, None,
                                     roots.ctypes.data, ns.ctypes.data, len(ns), report.ctypes.data)

    @staticmethod
    def entries(L, h, first, k):
        return L.qp_ballot_box_entries(h, first, k, None, None, None)

    @staticmethod
    def log(L, h, n):
        log = np.zeros((n, 4), np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
        assert L.qp_ballot_box_entries(h, 0, n, *(a.ctypes.data for a in log)) == 0
        return log

    @staticmethod
    def entries_at(L, h, seqs, k):
        return L.qp_ballot_box_entries_at(h, seqs, k, None, None, None)


class Ledger:
    abi, audit = "qp_ledger", "qp_ledger_log_audit"

    @staticmethod
    def open(ctx, capacity=CAPACITY):
        from qp_wormhole import WormholeLedger
        return WormholeLedger(ctx, [ROOT_A], capacity=capacity)

    @staticmethod
    def pis(nullifiers):
        return [transfer(q, amount=5 + i, account=(1, 2, 3, 4 + i % 2)) for i, q in enumerate(nullifiers)]

    @staticmethod
    def restore(L, c, capacity, log, cast_count, root, out):
        nul, num, amt, acc, fl = log
        return L.qp_ledger_restore(c, p64(*ROOT_A), 1, None, capacity, nul.ctypes.data, num.ctypes.data,
                                   amt.ctypes.data, acc.ctypes.data, fl.ctypes.data, len(num), cast_count, root, out)

    @staticmethod
    def audit_commitment(L, c, log, roots, ns, report):
        nul, num, amt, acc, fl = log
        return L.qp_ledger_log_audit(c, nul.ctypes.data, num.ctypes.data, amt.ctypes.data, acc.ctypes.data,
                                     fl.ctypes.data, len(num), None, None, None, None, None, 0, roots.ctypes.data,
                                     ns.ctypes.data, len(ns), report.ctypes.data)

    @staticmethod
    def entries(L, h, first, k):
        return L.qp_ledger_entries(h, first, k, None, None, None, None, None)

    @staticmethod
    def log(L, h, n):
        log = (np.zeros((n, 4), np.uint64), np.zeros(n, np.uint64), np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint64),
               np.zeros(n, np.uint8))
        assert L.qp_ledger_entries(h, 0, n, *(a.ctypes.data for a in log)) == 0
        return log

    @staticmethod
    def entries_at(L, h, seqs, k):
        return L.qp_ledger_entries_at(h, seqs, k, None, None, None, None, None)


class Env:
    """a handle with three admitted entries, an empty one, and the first one's published log"""

    def __init__(self, kind, ctx):
        from qp_wormhole import lib
        self.kind, self.L, self.c = kind, lib(), None if ctx is None else ctx.h
        self.full, self.empty = kind.open(ctx), kind.open(ctx)
        self.full.cast_public(kind.pis(NULLIFIERS[:ADMITTED]), reserve=False)
        assert self.full.admitted == ADMITTED and self.empty.admitted == 0
        self.log = kind.log(self.L, self.full.h, ADMITTED)
        self.sib = np.zeros((4, 32, 4), np.uint64)
        self.bits, self.depth = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
        self.out = np.zeros((4, 4), np.uint64)

    def call(self, name, h, *args):
        return getattr(self.L, f"{self.kind.abi}_{name}")(h.h, *args)

    def receipts(self, h, seqs, k):
        return self.call("receipts", h, seqs, k, self.sib.ctypes.data, self.bits.ctypes.data, self.depth.ctypes.data,
                         None, None, None)

    def restore(self, capacity=CAPACITY, log=None, cast_count=ADMITTED, root=None):
        h = ctypes.c_void_p()
        rc = self.kind.restore(self.L, self.c, capacity, self.log if log is None else log, cast_count, root,
                               ctypes.byref(h))
        assert rc and not h.value
        return rc

    def doubled(self):
        """the log with entry 2 a second, counted entry of entry 0's nullifier"""
        log = tuple(a.copy() for a in self.log)
        log[0][2] = log[0][0]
        return log

    def last_error(self, h):
        return getattr(self.L, f"{self.kind.abi}_last_error")(None if h is None else h.h).decode()


_ALIVE = []  # the arrays behind the pointers p64 gave out


def p64(*v):
    _ALIVE.append(u64(v))
    return _ALIVE[-1].ctypes.data


# (id, the call: Env -> (rc, the handle that carries the text or None), the code, the text after "<abi>");
# {e}: "ballot" / "transfer", {abi}: "qp_ballot_box" / "qp_ledger"
SHARED = [
    ("receipts_seq_outside", lambda v: (v.receipts(v.full, p64(0, 3), 2), v.full), ARG,
     "_receipts: entry 3 (position 1) is outside the log's 3"),
    ("entries_at_seq_outside", lambda v: (v.kind.entries_at(v.L, v.full.h, p64(5), 1), v.full), ARG,
     "_entries_at: entry 5 (position 0) is outside the log's 3"),
    ("commit_log_empty", lambda v: (v.call("commit_log", v.empty, None, None), v.empty), STATE,
     "_commit_log: empty log (no {e} has been admitted yet)"),
    ("receipts_empty", lambda v: (v.receipts(v.empty, None, 0), v.empty), STATE,
     "_receipts: empty log (no {e} has been admitted yet)"),
    ("roots_at_empty", lambda v: (v.call("roots_at", v.empty, None, 0, None), v.empty), STATE,
     "_roots_at: empty log (no {e} has been admitted yet)"),
    ("roots_at_size_0", lambda v: (v.call("roots_at", v.full, p64(1, 0), 2, v.out.ctypes.data), v.full), ARG,
     "_roots_at: size 0 (position 1) is outside 1..3, the sizes the log has had"),
    ("roots_at_size_above_n", lambda v: (v.call("roots_at", v.full, p64(4), 1, v.out.ctypes.data), v.full), ARG,
     "_roots_at: size 4 (position 0) is outside 1..3, the sizes the log has had"),
    ("entries_past_the_end", lambda v: (v.kind.entries(v.L, v.full.h, 2, 2), v.full), ARG,
     "_entries: entries [2, 2 + 2) are outside the log's 3"),
    ("find_non_canonical", lambda v: (v.call("find", v.full, p64(1, 2, 3, 4, 1, 2, P, 4), 2, v.out.ctypes.data), v.full),
     ARG, "_find: nullifier at position 1 felt 2 is not a canonical field element"),
    ("receipts_null", lambda v: (v.receipts(v.full, None, 1), v.full), ARG, "_receipts: null buffer"),
    ("entries_at_null", lambda v: (v.kind.entries_at(v.L, v.full.h, None, 1), v.full), ARG, "_entries_at: null buffer"),
    ("roots_at_null", lambda v: (v.call("roots_at", v.full, p64(1), 1, None), v.full), ARG, "_roots_at: null buffer"),
    ("find_null", lambda v: (v.call("find", v.full, None, 1, v.out.ctypes.data), v.full), ARG, "_find: null buffer"),
    ("cast_public_null", lambda v: (v.call("cast_public", v.full, None, None, 1, None), v.full), ARG,
     "_cast_public: null buffer"),
    ("cast_public_over_capacity", lambda v: (v.call("cast_public", v.full, u64(v.kind.pis(NULLIFIERS[3:])).ctypes.data,
                                                    None, 6, np.zeros(6 * 3, np.uint64).ctypes.data), v.full), ARG,
     "_cast_public: 3 + 6 admitted {e}s exceed the capacity 8; call {abi}_reserve first"),
    ("reserve_below_admitted", lambda v: (v.call("reserve", v.full, 2), v.full), ARG,
     "_reserve: capacity 2 for 3 admitted {e}s: it must hold them (and at least one) and be at most 2^31"),
    ("restore_capacity_too_small", lambda v: (v.restore(capacity=2), None), ARG,
     "_restore: capacity 2 for a log of 3 entries: it must hold them (and at least one) and be at most 2^31"),
    ("restore_cast_count", lambda v: (v.restore(cast_count=2), None), ARG,
     "_restore: cast_count 2 is not above the log's last {e} number 2"),
    ("restore_expected_root_non_canonical", lambda v: (v.restore(root=p64(1, P, 3, 4)), None), ARG,
     "_restore: the expected root is not four canonical field elements"),
]
OWN = {
    Box: [
        ("restore_failing_audit", lambda v: (v.restore(log=v.doubled()), None), FORMAT,
         "qp_ballot_box_restore: the log fails its audit: the count rule is broken (entry 2, its nullifier first at entry 0)"),
        ("log_audit_commitment_n_0", lambda v: (v.kind.audit_commitment(v.L, v.c, v.log, u64([[1, 2, 3, 4]] * 2), u64([3, 0]),
                                                                        np.zeros(10, np.uint64)), None), ARG,
         "qp_ballot_log_audit: commitment 1 names n = 0"),
    ],
    Ledger: [
        ("restore_failing_audit", lambda v: (v.restore(log=v.doubled()), None), FORMAT,
         "qp_ledger_restore: the log fails its audit: credit rule broken (entry 2, its nullifier first at entry 0)"),
        ("log_audit_commitment_n_0", lambda v: (v.kind.audit_commitment(v.L, v.c, v.log, u64([[1, 2, 3, 4]] * 2), u64([3, 0]),
                                                                        np.zeros(13, np.uint64)), None), ARG,
         "qp_ledger_log_audit: commitment 1 names n = 0"),
        ("totals_for_non_canonical", lambda v: (v.call("totals_for", v.full, p64(P, 2, 3, 4), 1, None, None), v.full), ARG,
         "qp_ledger_totals_for: account at position 0 felt 0 is not a canonical field element"),
        ("totals_for_null", lambda v: (v.call("totals_for", v.full, None, 1, None, None), v.full), ARG,
         "qp_ledger_totals_for: null buffer"),
    ],
}
NOUN = {Box: "ballot", Ledger: "transfer"}
CASES = [(kind, name, call, rc, kind.abi + text.format(e=NOUN[kind], abi=kind.abi))
         for kind in (Box, Ledger) for name, call, rc, text in SHARED] + \
        [(kind, name, call, rc, text) for kind in (Box, Ledger) for name, call, rc, text in OWN[kind]]
IDS = [f"{kind.__name__.lower()}-{name}" for kind, name, _, _, _ in CASES]


def check_case(env, call, rc, text):
    got, carrier = call(env)
    assert (got, env.last_error(carrier)) == (rc, text)
    assert env.full.admitted == ADMITTED and env.full.capacity == CAPACITY  # a refusal changes nothing


@pytest.fixture(scope="module")
def envs():
    return {kind: Env(kind, None) for kind in (Box, Ledger)}


@pytest.mark.parametrize("kind,name,call,rc,text", CASES, ids=IDS)
def test_refusal(envs, kind, name, call, rc, text):
    check_case(envs[kind], call, rc, text)
