"""CPU-side checks of the ledger's log-commitment and audit part of the C ABI
through ctypes on the host path: the entry points are declared, exported and
bound with the header's arity; null pointers are refused; k = 0 is accepted;
qp_ledger_receipt_check returns each reason code; qp_ledger_log_audit's
argument errors are QP_ERR_ARG and not a verdict."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole
from qp_wormhole.ledger import LEDGER_AUDIT_DTYPE, RESULT_DTYPE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")
P = 0xFFFFFFFF00000001
ROOT = np.array([5, 6, 7, 8], np.uint64)
OK, SHAPE, ROOT_MISMATCH, NON_CANONICAL, NULL = range(5)

SYMBOLS = {"qp_ledger_commit_log": 3, "qp_ledger_entries_at": 8, "qp_ledger_receipts": 9, "qp_ledger_roots_at": 4,
           "qp_ledger_receipt_check": 11, "qp_ledger_log_audit": 17}


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
    enum = re.search(r"typedef enum \{([^}]*)\} qp_ledger_audit_status;", txt, re.S).group(1)
    assert re.findall(r"QP_LEDGER_AUDIT_(\w+) = (\d+)", enum) == [
        ("OK", "0"), ("NON_CANONICAL", "1"), ("ORDER", "2"), ("CREDIT_RULE", "3"), ("TOTALS", "4"), ("PAYOUTS", "5"),
        ("ROOT", "6"), ("COMMITMENT", "7")]
    assert len(qp_wormhole.LEDGER_AUDIT_STATUS_TEXT) == 8 and LEDGER_AUDIT_DTYPE.itemsize == 104


def ledger_with(n, capacity=8):
    """a host ledger holding n transfers: nullifier [9, 9, 9, i], amount limbs [0, 0, i, 7], account [4, 4, 4, i & 1]"""
    L = qp_wormhole.lib()
    h = ctypes.c_void_p()
    assert L.qp_ledger_new(None, ROOT.ctypes.data, 1, None, capacity, ctypes.byref(h)) == 0
    if n:
        pis = np.array([[9, 9, 9, i] + list(ROOT) + [0, 0, i, 7] + [4, 4, 4, i & 1] for i in range(n)], np.uint64)
        res = np.zeros(n, RESULT_DTYPE)
        assert L.qp_ledger_cast_public(h, pis.ctypes.data, None, n, res.ctypes.data) == 0
    return L, h


def test_null_pointers_and_k_zero():
    L, h = ledger_with(3)
    try:
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        sib = np.zeros((1, 32, 4), np.uint64)
        bits, depth = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        seqs, ms, out = np.array([1], np.uint64), np.array([2], np.uint64), np.zeros(4, np.uint64)
        # null handles
        assert L.qp_ledger_commit_log(None, root.ctypes.data, ctypes.byref(n)) == 1
        assert L.qp_ledger_receipts(None, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                    None, None, None) == 1
        assert L.qp_ledger_entries_at(None, seqs.ctypes.data, 1, None, None, None, None, None) == 1
        assert L.qp_ledger_roots_at(None, ms.ctypes.data, 1, out.ctypes.data) == 1
        # null buffers with k > 0
        for args in ((None, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data),
                     (seqs.ctypes.data, 1, None, bits.ctypes.data, depth.ctypes.data),
                     (seqs.ctypes.data, 1, sib.ctypes.data, None, depth.ctypes.data),
                     (seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, None)):
            assert L.qp_ledger_receipts(h, *args, None, None, None) == 1
            assert b"null buffer" in L.qp_ledger_last_error(h)
        assert L.qp_ledger_entries_at(h, None, 1, None, None, None, None, None) == 1
        assert L.qp_ledger_roots_at(h, None, 1, out.ctypes.data) == 1
        assert L.qp_ledger_roots_at(h, ms.ctypes.data, 1, None) == 1
        # k == 0 is QP_OK whatever the pointers; receipts still commits and reports the pair
        assert L.qp_ledger_entries_at(h, None, 0, None, None, None, None, None) == 0
        assert L.qp_ledger_roots_at(h, None, 0, None) == 0
        assert L.qp_ledger_receipts(h, None, 0, None, None, None, None, root.ctypes.data, ctypes.byref(n)) == 0
        assert n.value == 3 and root.any()
        # the optional outputs may be null
        assert L.qp_ledger_commit_log(h, None, None) == 0
        assert L.qp_ledger_entries_at(h, seqs.ctypes.data, 1, None, None, None, None, None) == 0
        assert L.qp_ledger_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                    None, None, None) == 0
        assert (int(depth[0]), int(bits[0])) == (2, 1)  # entry 1 of 3: a right child, then a left one
        assert L.qp_ledger_roots_at(h, ms.ctypes.data, 1, out.ctypes.data) == 0 and out.any()
        # an entry outside the log, a size the log never had
        seqs[0] = 3
        assert L.qp_ledger_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                    None, None, None) == 1
        assert b"position 0" in L.qp_ledger_last_error(h)
        assert L.qp_ledger_entries_at(h, seqs.ctypes.data, 1, None, None, None, None, None) == 1
        for m in (0, 4):
            ms[0] = m
            assert L.qp_ledger_roots_at(h, ms.ctypes.data, 1, out.ctypes.data) == 1
    finally:
        L.qp_ledger_free(h)
    L, h = ledger_with(0)
    try:
        assert L.qp_ledger_commit_log(h, None, None) == 4
        assert b"empty log" in L.qp_ledger_last_error(h)
        assert L.qp_ledger_receipts(h, None, 0, None, None, None, None, None, None) == 4
        assert L.qp_ledger_roots_at(h, None, 0, None) == 4
    finally:
        L.qp_ledger_free(h)


def test_receipt_check_reason_codes():
    L, h = ledger_with(5)
    try:
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        seqs = np.array([2], np.uint64)
        sib = np.zeros((32, 4), np.uint64)
        bits, depth = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        nul, acc, num = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(1, np.uint64)
        amt, fl = np.zeros(4, np.uint32), np.zeros(1, np.uint8)
        assert L.qp_ledger_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                    None, root.ctypes.data, ctypes.byref(n)) == 0
        assert L.qp_ledger_entries_at(h, seqs.ctypes.data, 1, nul.ctypes.data, num.ctypes.data, amt.ctypes.data,
                                      acc.ctypes.data, fl.ctypes.data) == 0
        assert (list(nul), int(num[0]), list(amt), list(acc), int(fl[0]), n.value) == \
            ([9, 9, 9, 2], 2, [0, 0, 2, 7], [4, 4, 4, 0], 1, 5)
        d, b = int(depth[0]), int(bits[0])
        assert (d, b) == (3, 0b010)  # entry 2 of 5: left, right, left

        def check(root=root, n=5, seq=2, nul=nul, number=2, amt=amt, acc=acc, flags=1, sib=sib, bits=b, depth=d):
            p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
            return L.qp_ledger_receipt_check(p(root), n, seq, p(nul), number, p(amt), p(acc), flags, p(sib), bits, depth)
        assert check() == OK
        assert check(root=None) == check(nul=None) == check(sib=None) == check(amt=None) == check(acc=None) == NULL
        # shape: seq and n, the depth, a side bit, a non-zero slot above the depth
        assert check(seq=5) == check(n=0) == check(n=2**31 + 1) == SHAPE
        assert check(depth=d - 1) == check(depth=d + 1) == check(depth=33) == check(bits=b ^ 2) == SHAPE
        assert check(n=4) == SHAPE  # four leaves give entry 2 a path of two
        dirty = sib.copy()
        dirty[d, 0] = 1
        assert check(sib=dirty) == SHAPE
        # root: each part of the entry, a sibling, the root itself
        assert check(flags=0) == check(number=3) == ROOT_MISMATCH
        for arr, name in ((nul, "nul"), (acc, "acc"), (amt, "amt")):
            for j in range(4):
                other = arr.copy()
                other[j] ^= 1
                assert check(**{name: other}) == ROOT_MISMATCH, (name, j)
        assert check(amt=np.array([0, 2, 0, 7], np.uint32)) == ROOT_MISMATCH  # two limbs swapped
        wrong = sib.copy()
        wrong[0, 1] ^= 1
        assert check(sib=wrong) == check(root=ROOT) == ROOT_MISMATCH
        # a felt >= p, or a flags byte that is none of the log's
        for name in ("root", "nul", "acc", "sib"):
            bad = {"root": root, "nul": nul, "acc": acc, "sib": sib}[name].copy()
            bad.reshape(-1)[1] = P
            assert check(**{name: bad}) == NON_CANONICAL, name
        assert check(number=P) == check(flags=2) == NON_CANONICAL
    finally:
        L.qp_ledger_free(h)


def test_audit_argument_errors_are_not_verdicts():
    L, h = ledger_with(4)
    try:
        nul, acc, num = np.zeros((4, 4), np.uint64), np.zeros((4, 4), np.uint64), np.zeros(4, np.uint64)
        amt, fl = np.zeros((4, 4), np.uint32), np.zeros(4, np.uint8)
        assert L.qp_ledger_entries(h, 0, 4, nul.ctypes.data, num.ctypes.data, amt.ctypes.data, acc.ctypes.data,
                                   fl.ctypes.data) == 0
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        assert L.qp_ledger_commit_log(h, root.ctypes.data, ctypes.byref(n)) == 0
        pa, ps, pf = np.zeros((2, 4), np.uint64), np.zeros((2, 4), np.uint64), np.zeros(2, np.uint64)
        assert L.qp_ledger_payouts(h, 0, 2, pa.ctypes.data, ps.ctypes.data, pf.ctypes.data) == 0
        tot = np.zeros(6, np.uint64)
        assert L.qp_ledger_recount(h, tot.ctypes.data) == 0
    finally:
        L.qp_ledger_free(h)
    totals = np.concatenate([tot[:1], tot[2:]])
    out = np.zeros(1, LEDGER_AUDIT_DTYPE)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def audit(nul=nul, num=num, amt=amt, acc=acc, fl=fl, n=4, root=root, totals=totals, pa=pa, ps=ps, pf=pf, npay=2,
              cr=root, cn=np.array([4], np.uint64), nc=1, out=out):
        return L.qp_ledger_log_audit(None, p(nul), p(num), p(amt), p(acc), p(fl), n, p(root), p(totals), p(pa), p(ps),
                                     p(pf), npay, p(cr), p(cn), nc, p(out))
    assert audit() == 0 and out[0]["status"] == 0 and out[0]["root"].tolist() == root.tolist()
    assert (int(out[0]["credited"]), out[0]["sums"].tolist(), int(out[0]["accounts"])) == (4, [0, 0, 6, 28], 2)
    assert int(out[0]["witness"]) == int(out[0]["first"]) == 2**64 - 1
    # nothing claimed at all is an audit too
    assert audit(root=None, totals=None, pa=None, ps=None, pf=None, npay=0, cr=None, cn=None, nc=0) == 0
    assert out[0]["status"] == 0
    assert audit(out=None) == 1
    for name in ("nul", "num", "amt", "acc", "fl"):
        assert audit(**{name: None}) == 1, name
        assert b"null buffer" in L.qp_ledger_last_error(None)
    assert audit(n=0) == audit(n=2**31 + 1) == 1
    assert audit(ps=None) == audit(pf=None) == audit(cr=None) == audit(cn=None) == 1
    bad = root.copy()
    bad[2] = P
    assert audit(root=bad) == audit(cr=bad) == 1
    bad = pa.copy()
    bad[1, 3] = P
    assert audit(pa=bad) == 1 and b"claimed payout 1" in L.qp_ledger_last_error(None)
    assert audit(cn=np.array([0], np.uint64)) == 1 and b"n = 0" in L.qp_ledger_last_error(None)
    # a non-canonical *entry* is a verdict, with nothing hashed
    bad = acc.copy()
    bad[2, 0] = P
    assert audit(acc=bad) == 0
    assert (int(out[0]["status"]), int(out[0]["witness"]), out[0]["root"].tolist(), int(out[0]["credited"])) == \
        (1, 2, [0, 0, 0, 0], 0)


def test_raw_payouts_are_taken_whole_or_refused():
    """the raw form of the payouts goes to the audit as the arrays it is, an empty list included; arrays
    of unequal length or another type are a ValueError before anything is read"""
    import pytest
    from qp_wormhole import WormholeLedger, audit_ledger_log
    led = WormholeLedger(None, [ROOT.tolist()], capacity=8)
    try:
        pis = np.array([[9, 9, 9, i] + list(ROOT) + [0, 0, i, 7] + [4, 4, 4, i & 1] for i in range(4)], np.uint64)
        led.cast_public(pis, raw=True)
        entries, (a, s, f) = led.entries(), led.payouts(raw=True)
    finally:
        led.free()
    assert audit_ledger_log(None, entries, payouts=(a, s, f)).status == 0
    rep = audit_ledger_log(None, entries, payouts=(a[:0], s[:0], f[:0]))
    assert (rep.status, rep.witness) == (5, 0)
    rep = audit_ledger_log(None, entries, payouts=(a[::-1], s[::-1], f[::-1]))  # not contiguous as given
    assert (rep.status, rep.witness) == (5, 0)
    for bad in ((a[:1], s, f), (a, s[:1], f), (a, s, f[:1]), (a, s.astype(np.int64), f), (a, s, f.reshape(-1, 1))):
        with pytest.raises(ValueError, match="raw payouts"):
            audit_ledger_log(None, entries, payouts=bad)
