"""CPU-side checks of the transfer-ledger part of the C ABI: include/qpgpu.h
declares the entry points, libqpgpu.so exports them, the ctypes table binds
them with the header's arity, and every refusal is a status that leaves the
ledger as it was (host ledgers: no device needed)."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")
P = 0xFFFFFFFF00000001
ROOT = np.array([5, 6, 7, 8], np.uint64)

# name -> number of parameters in include/qpgpu.h
SYMBOLS = {"qp_ledger_new": 6, "qp_ledger_free": 1, "qp_ledger_last_error": 1, "qp_ledger_accept_root": 2,
           "qp_ledger_reserve": 2, "qp_ledger_state": 6, "qp_ledger_cast": 6, "qp_ledger_cast_public": 5,
           "qp_ledger_find": 4, "qp_ledger_entries": 8, "qp_ledger_payouts": 6, "qp_ledger_totals_for": 5,
           "qp_ledger_recount": 2, "qp_ledger_cast_times": 2}


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
    for name in ("WormholeLedger", "TransferResult", "TRANSFER_STATUS_TEXT"):
        assert name in qp_wormhole.__all__ and hasattr(qp_wormhole, name)
    assert qp_wormhole.WormholeLedger.__module__ == "qp_wormhole.ledger"
    # the status enum's values are the Python table's order
    enum = re.search(r"typedef enum \{([^}]*)\} qp_transfer_status;", txt).group(1)
    names = re.findall(r"QP_TRANSFER_(\w+) = (\d+)", enum)
    assert [int(v) for _, v in names] == list(range(7)) and len(qp_wormhole.TRANSFER_STATUS_TEXT) == 7
    assert [n for n, _ in names] == ["CREDITED", "PROOF_REJECTED", "MALFORMED", "PADDING", "BAD_AMOUNT", "UNKNOWN_ROOT",
                                     "DOUBLE_SPEND"]


def new_ledger(capacity=4, roots=ROOT, nroots=1, padding=None):
    h = ctypes.c_void_p()
    rc = qp_wormhole.lib().qp_ledger_new(None, None if roots is None else roots.ctypes.data, nroots,
                                         None if padding is None else padding.ctypes.data, capacity, ctypes.byref(h))
    return rc, h


def test_null_handles_are_argument_errors():
    L = qp_wormhole.lib()
    out = np.zeros(6, np.uint64)
    assert L.qp_ledger_accept_root(None, ROOT.ctypes.data) == 1
    assert L.qp_ledger_cast(None, None, None, None, 0, None) == 1
    assert L.qp_ledger_cast_public(None, None, None, 0, None) == 1
    assert L.qp_ledger_reserve(None, 8) == 1
    assert L.qp_ledger_state(None, None, None, None, None, None) == 1
    assert L.qp_ledger_find(None, None, 0, None) == 1
    assert L.qp_ledger_entries(None, 0, 0, None, None, None, None, None) == 1
    assert L.qp_ledger_payouts(None, 0, 0, None, None, None) == 1
    assert L.qp_ledger_totals_for(None, None, 0, None, None) == 1
    assert L.qp_ledger_recount(None, out.ctypes.data) == 1
    assert L.qp_ledger_cast_times(None, None) == 1
    L.qp_ledger_free(None)
    assert L.qp_ledger_new(None, ROOT.ctypes.data, 1, None, 4, None) == 1


def test_new_refusals_name_their_reason():
    L = qp_wormhole.lib()
    roots4097 = np.ones((4097, 4), np.uint64)
    for kw, word in ((dict(capacity=0), b"capacity"), (dict(capacity=(1 << 31) + 1), b"capacity"),
                     (dict(nroots=0), b"0 accepted roots"), (dict(roots=roots4097, nroots=4097), b"4097 accepted roots"),
                     (dict(roots=None), b"null roots"),
                     (dict(roots=np.array([1, 2, 3, P], np.uint64)), b"root"),
                     (dict(padding=np.array([1] * 15 + [P], np.uint64)), b"padding")):
        rc, h = new_ledger(**kw)
        assert rc == 1 and not h.value, kw
        assert word in L.qp_ledger_last_error(None), kw
    rc, h = new_ledger(capacity=1)  # the smallest ledger: one entry, two slots per table
    assert rc == 0 and h.value
    L.qp_ledger_free(h)
    # a root given twice is held once: 4096 copies and one other are two roots
    roots = np.tile(ROOT, (4096, 1))
    roots[-1, 0] = 9
    rc, h = new_ledger(roots=roots, nroots=4096)
    assert rc == 0
    for i in range(4094):
        assert L.qp_ledger_accept_root(h, np.array([i, 1, 1, 1], np.uint64).ctypes.data) == 0
    assert L.qp_ledger_accept_root(h, np.array([5000, 1, 1, 1], np.uint64).ctypes.data) == 1
    L.qp_ledger_free(h)


def state(L, h):
    v = [ctypes.c_uint64() for _ in range(5)]
    assert L.qp_ledger_state(h, *[ctypes.byref(x) for x in v]) == 0
    rec = np.zeros(6, np.uint64)
    assert L.qp_ledger_recount(h, rec.ctypes.data) == 0
    return tuple(x.value for x in v) + tuple(int(x) for x in rec)


def row(i, account=3):
    return [9, 9, 9, i] + list(ROOT) + [0, 0, 0, 10 + i] + [account, 0, 0, 0]


def test_refused_calls_change_nothing_and_n_zero_is_ok():
    L = qp_wormhole.lib()
    rc, h = new_ledger(capacity=2)
    assert rc == 0
    try:
        res = np.zeros(3, qp_wormhole.ledger.RESULT_DTYPE)
        pis = np.array([row(i) for i in range(3)], np.uint64)
        empty = (0, 0, 0, 0, 2) + (0,) * 6
        # n == 0 is QP_OK whatever the pointers
        assert L.qp_ledger_cast_public(h, None, None, 0, None) == 0
        assert state(L, h) == empty
        # null buffers with n > 0
        assert L.qp_ledger_cast_public(h, None, None, 1, res.ctypes.data) == 1
        assert L.qp_ledger_cast_public(h, pis.ctypes.data, None, 1, None) == 1
        # more than 2^22 transfers in one call: refused on the length alone, no buffer is read
        assert L.qp_ledger_cast_public(h, pis.ctypes.data, None, (1 << 22) + 1, res.ctypes.data) == 1
        assert b"2^22" in L.qp_ledger_last_error(h)
        # three admitted transfers into a capacity of two: refused whole
        assert L.qp_ledger_cast_public(h, pis.ctypes.data, None, 3, res.ctypes.data) == 1
        assert b"qp_ledger_reserve" in L.qp_ledger_last_error(h)
        assert state(L, h) == empty
        assert L.qp_ledger_cast_public(h, pis.ctypes.data, None, 2, res.ctypes.data) == 0
        assert [tuple(r) for r in res[:2]] == [(0, 0, 0, 0), (0, 0, 1, 1)]
        full = (2, 2, 2, 1, 2, 2, 2, 0, 0, 0, 21)
        assert state(L, h) == full
        # a full ledger still takes transfers that are not admitted, and numbers them
        verdicts = np.array([7], np.uint32)
        assert L.qp_ledger_cast_public(h, pis[2:].ctypes.data, verdicts.ctypes.data, 1, res.ctypes.data) == 0
        assert tuple(res[0]) == (1, 7, 2, 2)
        assert L.qp_ledger_cast_public(h, pis[2:].ctypes.data, None, 1, res.ctypes.data) == 1
        full = (3,) + full[1:]
        assert state(L, h) == full
        # cast: a null verifier, and n == 0 checked after it
        assert L.qp_ledger_cast(h, None, None, None, 0, None) == 1
        assert b"verifier" in L.qp_ledger_last_error(h)
        # entries and payouts outside what there is; reserve below the admitted count or above 2^31
        assert L.qp_ledger_entries(h, 1, 2, None, None, None, None, None) == 1
        assert L.qp_ledger_entries(h, 3, 0, None, None, None, None, None) == 1
        assert L.qp_ledger_entries(h, 2, 0, None, None, None, None, None) == 0
        amt = np.zeros((2, 4), np.uint32)
        assert L.qp_ledger_entries(h, 0, 2, None, None, amt.ctypes.data, None, None) == 0
        assert amt.tolist() == [[0, 0, 0, 10], [0, 0, 0, 11]]
        assert L.qp_ledger_payouts(h, 0, 2, None, None, None) == 1
        assert L.qp_ledger_payouts(h, 2, 0, None, None, None) == 1
        sums, seq = np.zeros(4, np.uint64), np.zeros(1, np.uint64)
        assert L.qp_ledger_payouts(h, 0, 1, None, sums.ctypes.data, seq.ctypes.data) == 0
        assert list(sums) == [0, 0, 0, 21] and seq[0] == 0
        # null or non-canonical keys
        one = np.zeros(1, np.uint64)
        assert L.qp_ledger_find(h, None, 1, one.ctypes.data) == 1
        assert L.qp_ledger_find(h, pis.ctypes.data, 1, None) == 1
        assert L.qp_ledger_totals_for(h, None, 1, None, None) == 1
        bad = np.array([1, 2, 3, P], np.uint64)
        assert L.qp_ledger_find(h, bad.ctypes.data, 1, one.ctypes.data) == 1
        assert L.qp_ledger_totals_for(h, bad.ctypes.data, 1, None, None) == 1
        assert L.qp_ledger_find(h, pis[1].ctypes.data, 1, one.ctypes.data) == 0 and one[0] == 1
        assert L.qp_ledger_find(h, pis[2].ctypes.data, 1, one.ctypes.data) == 0 and one[0] == 2**64 - 1
        found = np.ones(1, np.uint8)
        assert L.qp_ledger_totals_for(h, np.array([4, 0, 0, 0], np.uint64).ctypes.data, 1, sums.ctypes.data,
                                      found.ctypes.data) == 0
        assert list(sums) == [0, 0, 0, 0] and found[0] == 0
        assert L.qp_ledger_reserve(h, 1) == 1
        assert L.qp_ledger_reserve(h, (1 << 31) + 1) == 1
        assert L.qp_ledger_reserve(h, 2) == 0
        assert L.qp_ledger_accept_root(h, bad.ctypes.data) == 1
        assert L.qp_ledger_accept_root(h, None) == 1
        assert L.qp_ledger_recount(h, None) == 1
        assert state(L, h) == full
        assert L.qp_ledger_reserve(h, 3) == 0
        assert L.qp_ledger_cast_public(h, pis[2:].ctypes.data, None, 1, res.ctypes.data) == 0
        assert tuple(res[0]) == (0, 0, 3, 3) and state(L, h) == (4, 3, 3, 1, 3, 3, 3, 0, 0, 0, 33)
        ms = (ctypes.c_double * 2)(1, 1)
        assert L.qp_ledger_cast_times(h, ms) == 0 and list(ms) == [0, 0]
    finally:
        L.qp_ledger_free(h)


def test_a_verifier_of_a_13_input_circuit_is_refused():
    """qp_ledger_cast takes a verifier of a circuit with 16 public inputs: the voting
    circuit's (13) is an argument error, checked before the proofs are looked at"""
    import pytest
    from qp_wormhole import Circuit, QpError, WormholeLedger, WormholeVerifier
    circ = Circuit.voting()
    cb = circ.common_data()
    ver = None
    for h in range(17):  # a well-formed all-zero VerifierOnlyCircuitData of the common data's cap height
        try:
            ver = WormholeVerifier(circuit_data=((h).to_bytes(8, "little") + bytes(32 * (1 << h) + 32), cb), device=None,
                                   max_batch=1)
            break
        except QpError as e:
            assert "cap height" in str(e)
    assert ver is not None
    led = WormholeLedger(None, [list(ROOT)], verifier=ver, capacity=4)
    try:
        led.cast_public([row(0)])
        with pytest.raises(QpError, match="QP_ERR_ARG.*13 public inputs"):
            led.cast([b"not looked at"])
        assert (led.cast_count, led.admitted, led.credited) == (1, 1, 1)
    finally:
        led.free()
        ver.close()
        circ.free()
