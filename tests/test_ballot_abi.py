"""CPU-side checks of the ballot-box part of the C ABI: include/qpgpu.h declares
the entry points, libqpgpu.so exports them, the ctypes table binds them with
the header's arity, and every refusal is a status that leaves the box as it
was (host boxes: no device needed)."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")
P = 0xFFFFFFFF00000001
PROPOSAL = np.array([1, 2, 3, 4], np.uint64)
ROOT = np.array([5, 6, 7, 8], np.uint64)

# name -> number of parameters in include/qpgpu.h
SYMBOLS = {"qp_ballot_box_new": 6, "qp_ballot_box_free": 1, "qp_ballot_box_last_error": 1,
           "qp_ballot_box_accept_root": 2, "qp_ballot_box_cast": 6, "qp_ballot_box_cast_public": 5,
           "qp_ballot_box_reserve": 2, "qp_ballot_box_tally": 3, "qp_ballot_box_state": 4, "qp_ballot_box_entries": 6,
           "qp_ballot_box_recount": 2, "qp_ballot_box_cast_times": 2}


def test_symbols_declared_exported_and_bound():
    L = qp_wormhole.lib()
    declared = qp_wormhole.header_symbols()
    txt = open(HEADER).read()
    for s, arity in SYMBOLS.items():
        assert s in declared, s
        f = getattr(L, s)
        assert f.argtypes is not None and len(f.argtypes) == arity, s
        m = re.search(r"^[\w ]+?\*?%s\s*\(([^)]*)\)\s*;" % s, txt, re.M)
        assert m and len(m.group(1).split(",")) == arity, s
    for name in ("BallotBox", "BallotResult", "BALLOT_STATUS_TEXT"):
        assert name in qp_wormhole.__all__ and hasattr(qp_wormhole, name)
    assert qp_wormhole.BallotBox.__module__ == "qp_wormhole.ballot"
    # the status enum's values are the Python table's order
    enum = re.search(r"typedef enum \{([^}]*)\} qp_ballot_status;", txt).group(1)
    names = re.findall(r"QP_BALLOT_(\w+) = (\d+)", enum)
    assert [int(v) for _, v in names] == list(range(7)) and len(qp_wormhole.BALLOT_STATUS_TEXT) == 7
    assert [n for n, _ in names] == ["COUNTED", "PROOF_REJECTED", "MALFORMED", "WRONG_PROPOSAL", "UNKNOWN_ROOT",
                                     "BAD_VOTE", "DOUBLE_VOTE"]


def new_box(capacity=4, proposal=PROPOSAL, roots=ROOT, nroots=1):
    h = ctypes.c_void_p()
    rc = qp_wormhole.lib().qp_ballot_box_new(None, proposal, roots, nroots, capacity, ctypes.byref(h))
    return rc, h


def test_null_handles_are_argument_errors():
    L = qp_wormhole.lib()
    out = np.zeros(4, np.uint64)
    assert L.qp_ballot_box_accept_root(None, ROOT) == 1
    assert L.qp_ballot_box_cast(None, None, None, None, 0, None) == 1
    assert L.qp_ballot_box_cast_public(None, None, None, 0, None) == 1
    assert L.qp_ballot_box_reserve(None, 8) == 1
    assert L.qp_ballot_box_tally(None, None, None) == 1
    assert L.qp_ballot_box_state(None, None, None, None) == 1
    assert L.qp_ballot_box_entries(None, 0, 0, None, None, None) == 1
    assert L.qp_ballot_box_recount(None, out) == 1
    assert L.qp_ballot_box_cast_times(None, None) == 1
    L.qp_ballot_box_free(None)
    assert L.qp_ballot_box_new(None, PROPOSAL, ROOT, 1, 4, None) == 1


def test_new_refusals_name_their_reason():
    L = qp_wormhole.lib()
    roots65 = np.ones((65, 4), np.uint64)
    for kw, word in ((dict(capacity=0), b"capacity"), (dict(capacity=(1 << 31) + 1), b"capacity"),
                     (dict(nroots=0), b"0 accepted roots"), (dict(roots=roots65, nroots=65), b"65 accepted roots"),
                     (dict(proposal=np.array([1, 2, 3, P], np.uint64)), b"proposal_id"),
                     (dict(roots=np.array([1, 2, 3, P], np.uint64)), b"root")):
        rc, h = new_box(**kw)
        assert rc == 1 and not h.value, kw
        assert word in L.qp_ballot_box_last_error(None), kw
    rc, h = new_box(capacity=1)  # the smallest box: one entry, two slots
    assert rc == 0 and h.value
    L.qp_ballot_box_free(h)


def state(L, h):
    c, a, cap, y, n = (ctypes.c_uint64() for _ in range(5))
    assert L.qp_ballot_box_state(h, ctypes.byref(c), ctypes.byref(a), ctypes.byref(cap)) == 0
    assert L.qp_ballot_box_tally(h, ctypes.byref(y), ctypes.byref(n)) == 0
    return c.value, a.value, cap.value, y.value, n.value


def test_refused_calls_change_nothing_and_n_zero_is_ok():
    L = qp_wormhole.lib()
    rc, h = new_box(capacity=2)
    assert rc == 0
    try:
        res = np.zeros(3, qp_wormhole.ballot.RESULT_DTYPE)
        pis = np.array([list(PROPOSAL) + list(ROOT) + [i & 1, 9, 9, 9, i] for i in range(3)], np.uint64)
        # n == 0 is QP_OK whatever the pointers
        assert L.qp_ballot_box_cast_public(h, None, None, 0, None) == 0
        assert state(L, h) == (0, 0, 2, 0, 0)
        # null buffers with n > 0
        assert L.qp_ballot_box_cast_public(h, None, None, 1, res.ctypes.data) == 1
        assert L.qp_ballot_box_cast_public(h, pis.ctypes.data, None, 1, None) == 1
        # three admitted ballots into a capacity of two: refused whole
        assert L.qp_ballot_box_cast_public(h, pis.ctypes.data, None, 3, res.ctypes.data) == 1
        assert b"qp_ballot_box_reserve" in L.qp_ballot_box_last_error(h)
        assert state(L, h) == (0, 0, 2, 0, 0)
        assert L.qp_ballot_box_cast_public(h, pis.ctypes.data, None, 2, res.ctypes.data) == 0
        assert [tuple(r) for r in res[:2]] == [(0, 0, 0, 0), (0, 0, 1, 1)]
        assert state(L, h) == (2, 2, 2, 1, 1)
        # a full box still takes ballots that are not admitted, and numbers them
        verdicts = np.array([7], np.uint32)
        assert L.qp_ballot_box_cast_public(h, pis[2:].ctypes.data, verdicts.ctypes.data, 1, res.ctypes.data) == 0
        assert tuple(res[0]) == (1, 7, 2, 2)
        assert L.qp_ballot_box_cast_public(h, pis[2:].ctypes.data, None, 1, res.ctypes.data) == 1
        assert state(L, h) == (3, 2, 2, 1, 1)
        # cast: a null verifier, and n == 0 checked after it
        assert L.qp_ballot_box_cast(h, None, None, None, 0, None) == 1
        assert b"verifier" in L.qp_ballot_box_last_error(h)
        # entries outside the log; reserve below the admitted count or above 2^31
        assert L.qp_ballot_box_entries(h, 1, 2, None, None, None) == 1
        assert L.qp_ballot_box_entries(h, 3, 0, None, None, None) == 1
        assert L.qp_ballot_box_entries(h, 2, 0, None, None, None) == 0
        num = np.zeros(2, np.uint64)
        assert L.qp_ballot_box_entries(h, 0, 2, None, num.ctypes.data, None) == 0 and list(num) == [0, 1]
        assert L.qp_ballot_box_reserve(h, 1) == 1
        assert L.qp_ballot_box_reserve(h, (1 << 31) + 1) == 1
        assert L.qp_ballot_box_reserve(h, 2) == 0
        assert L.qp_ballot_box_accept_root(h, np.array([1, 2, 3, P], np.uint64)) == 1
        assert state(L, h) == (3, 2, 2, 1, 1)
        assert L.qp_ballot_box_reserve(h, 3) == 0
        assert L.qp_ballot_box_cast_public(h, pis[2:].ctypes.data, None, 1, res.ctypes.data) == 0
        assert tuple(res[0]) == (0, 0, 3, 3) and state(L, h) == (4, 3, 3, 1, 2)
        out = np.zeros(4, np.uint64)
        assert L.qp_ballot_box_recount(h, out) == 0 and list(out) == [1, 2, 3, 3]
        ms = (ctypes.c_double * 2)(1, 1)
        assert L.qp_ballot_box_cast_times(h, ms) == 0 and list(ms) == [0, 0]
    finally:
        L.qp_ballot_box_free(h)
