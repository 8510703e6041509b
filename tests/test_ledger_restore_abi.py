"""CPU-side checks of qp_ledger_restore, qp_ledger_payouts_between and
qp_ledger_log_payouts_between through ctypes on the host path: the entry points
are declared, exported and bound with the header's arity; null pointers and
every argument error are QP_ERR_ARG; a failing audit is QP_ERR_FORMAT and leaves
*out untouched."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole
from qp_wormhole.ledger import RESULT_DTYPE

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")
P = 0xFFFFFFFF00000001
ROOT = np.array([5, 6, 7, 8], np.uint64)
OK, ERR_ARG, ERR_FORMAT = 0, 1, 6
SENTINEL = 0x1234

SYMBOLS = {"qp_ledger_restore": 14, "qp_ledger_payouts_between": 8, "qp_ledger_log_payouts_between": 12}


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
    assert callable(qp_wormhole.ledger_log_payouts) and "ledger_log_payouts" in qp_wormhole.__all__
    assert callable(qp_wormhole.WormholeLedger.restore) and callable(qp_wormhole.WormholeLedger.payouts_between)


def published(n=6):
    """the log of a host ledger of n transfers, entry 4 a double spend of entry 1: (nul, num, amt, acc, fl)"""
    L = qp_wormhole.lib()
    h = ctypes.c_void_p()
    assert L.qp_ledger_new(None, ROOT.ctypes.data, 1, None, n, ctypes.byref(h)) == 0
    pis = np.array([[9, 9, 9, 1 if i == 4 else i] + list(ROOT) + [0, 0, i, 7] + [4, 4, 4, i & 1] for i in range(n)],
                   np.uint64)
    res = np.zeros(n, RESULT_DTYPE)
    assert L.qp_ledger_cast_public(h, pis.ctypes.data, None, n, res.ctypes.data) == 0
    nul, acc, num = np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64), np.zeros(n, np.uint64)
    amt, fl = np.zeros((n, 4), np.uint32), np.zeros(n, np.uint8)
    assert L.qp_ledger_entries(h, 0, n, nul.ctypes.data, num.ctypes.data, amt.ctypes.data, acc.ctypes.data,
                               fl.ctypes.data) == 0
    root = np.zeros(4, np.uint64)
    assert L.qp_ledger_commit_log(h, root.ctypes.data, None) == 0
    L.qp_ledger_free(h)
    assert fl.tolist() == [1, 1, 1, 1, 0, 1]
    return nul, num, amt, acc, fl, root


def test_restore_arguments_and_format():
    L = qp_wormhole.lib()
    nul, num, amt, acc, fl, root = published()
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def restore(roots=ROOT, nroots=1, padding=None, capacity=6, nul=nul, num=num, amt=amt, acc=acc, fl=fl, n=6,
                cast_count=6, expect=root, out="sentinel"):
        h = ctypes.c_void_p(SENTINEL)
        rc = L.qp_ledger_restore(None, p(roots), nroots, p(padding), capacity, p(nul), p(num), p(amt), p(acc), p(fl), n,
                                 cast_count, p(expect), None if out is None else ctypes.byref(h))
        if rc == OK:
            assert h.value not in (None, SENTINEL)
            state = [ctypes.c_uint64() for _ in range(5)]
            assert L.qp_ledger_state(h, *[ctypes.byref(x) for x in state]) == 0
            L.qp_ledger_free(h)
            return OK, tuple(x.value for x in state)
        assert h.value == SENTINEL  # *out is written on QP_OK only
        return rc, L.qp_ledger_last_error(None).decode()

    assert restore() == (OK, (6, 6, 5, 2, 6))
    assert restore(expect=None, capacity=9, cast_count=100) == (OK, (100, 6, 5, 2, 9))
    assert restore(out=None)[0] == ERR_ARG
    # the refusals of qp_ledger_new
    bad_root = ROOT.copy()
    bad_root[0] = P
    pad = np.arange(16, dtype=np.uint64)
    pad[3] = P
    for kw, text in (({"roots": None}, "null roots"), ({"nroots": 0}, "accepted roots"), ({"nroots": 4097}, "accepted roots"),
                     ({"roots": bad_root}, "canonical"), ({"padding": pad}, "padding"),
                     ({"capacity": 2**31 + 1}, "capacity"), ({"capacity": 0}, "capacity")):
        rc, why = restore(**kw)
        assert rc == ERR_ARG and text in why, (kw, why)
    # null log buffers, capacity < n, cast_count <= numbers[n - 1], the expected root
    for name in ("nul", "num", "amt", "acc", "fl"):
        rc, why = restore(**{name: None})
        assert rc == ERR_ARG and "null log buffer" in why, name
    rc, why = restore(capacity=5)
    assert rc == ERR_ARG and "capacity 5 for a log of 6" in why
    rc, why = restore(cast_count=5)
    assert rc == ERR_ARG and "cast_count 5 is not above the log's last transfer number 5" in why
    assert restore(cast_count=0)[0] == ERR_ARG
    rc, why = restore(expect=bad_root)
    assert rc == ERR_ARG and "expected root" in why
    rc, why = restore(n=0, expect=root)
    assert rc == ERR_ARG and "empty log has no root" in why
    assert restore(n=2**31 + 1)[0] == ERR_ARG
    # n == 0: any cast_count, null log buffers allowed
    assert restore(n=0, nul=None, num=None, amt=None, acc=None, fl=None, cast_count=0, expect=None, capacity=1) == \
        (OK, (0, 0, 0, 0, 1))
    assert restore(n=0, cast_count=41, expect=None) == (OK, (41, 0, 0, 0, 6))
    # a failing audit: QP_ERR_FORMAT with the reason and the witness, *out untouched
    bad = acc.copy()
    bad[2, 0] = P
    assert restore(acc=bad) == (ERR_FORMAT, "qp_ledger_restore: the log fails its audit: non-canonical entry (entry 2)")
    bad = num.copy()
    bad[3] = bad[2]
    assert restore(num=bad) == (ERR_FORMAT,
                                "qp_ledger_restore: the log fails its audit: transfer numbers out of order (entry 3)")
    bad = fl.copy()
    bad[4] = 1
    assert restore(fl=bad) == (ERR_FORMAT, "qp_ledger_restore: the log fails its audit: credit rule broken (entry 4, "
                               "its nullifier first at entry 1)")
    bad[4], bad[0] = 0, 0
    assert restore(fl=bad) == (ERR_FORMAT, "qp_ledger_restore: the log fails its audit: credit rule broken (entry 0, "
                               "its nullifier first at entry 0)")
    bad = amt.copy()
    bad[4, 3] ^= 1
    assert restore(amt=bad) == (ERR_FORMAT, "qp_ledger_restore: the log fails its audit: claimed root differs")
    assert restore(amt=bad, expect=None)[0] == OK
    assert restore() == (OK, (6, 6, 5, 2, 6))


def test_payouts_between_arguments():
    L = qp_wormhole.lib()
    nul, num, amt, acc, fl, root = published()
    h = ctypes.c_void_p()
    assert L.qp_ledger_restore(None, ROOT.ctypes.data, 1, None, 8, nul.ctypes.data, num.ctypes.data, amt.ctypes.data,
                               acc.ctypes.data, fl.ctypes.data, 6, 6, root.ctypes.data, ctypes.byref(h)) == 0
    a, s, f = np.full((3, 4), 0xA5, np.uint64), np.full((3, 4), 0xA5, np.uint64), np.full(3, 0xA5, np.uint64)
    count = ctypes.c_uint64(77)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def ledger_form(m0, m1, cap, a, s, f, count):
        return L.qp_ledger_payouts_between(h, m0, m1, cap, p(a), p(s), p(f), None if count is None else ctypes.byref(count))

    def log_form(m0, m1, cap, a, s, f, count, acc=acc, amt=amt, fl=fl, n=6):
        return L.qp_ledger_log_payouts_between(None, p(acc), p(amt), p(fl), n, m0, m1, cap, p(a), p(s), p(f),
                                               None if count is None else ctypes.byref(count))
    try:
        assert L.qp_ledger_payouts_between(None, 0, 6, 0, None, None, None, ctypes.byref(count)) == ERR_ARG
        for form in (ledger_form, log_form):
            # out-of-range arguments, a null count, a null array with cap > 0: QP_ERR_ARG, nothing stored
            for args in ((3, 2, 3, a, s, f, count), (0, 7, 3, a, s, f, count), (7, 7, 3, a, s, f, count),
                         (0, 6, 3, a, s, f, None), (0, 6, 3, None, s, f, count), (0, 6, 3, a, None, f, count),
                         (0, 6, 3, a, s, None, count)):
                assert form(*args) == ERR_ARG, args
                assert count.value == 77 and (a == 0xA5).all() and (s == 0xA5).all() and (f == 0xA5).all()
            # m0 == m1: no rows, at either end of the log
            for m in (0, 3, 6):
                assert form(m, m, 3, a, s, f, count) == OK and count.value == 0 and (a == 0xA5).all()
                count.value = 77
            # the sizing call, then the filling call; entry 4 (a double spend) does not count
            assert form(0, 6, 0, None, None, None, count) == OK and count.value == 2
            assert form(0, 6, 3, a, s, f, count) == OK and count.value == 2
            assert a[:2].tolist() == [[4, 4, 4, 0], [4, 4, 4, 1]] and f[:2].tolist() == [0, 1] and (a[2] == 0xA5).all()
            assert s[:2].tolist() == [[0, 0, 0 + 2, 14], [0, 0, 1 + 3 + 5, 21]]
            # entries [3, 6): account 1 by entries 3 and 5; account 0's entry 4 is a double spend
            assert form(3, 6, 3, a, s, f, count) == OK and count.value == 1
            assert (a[0].tolist(), s[0].tolist(), int(f[0])) == ([4, 4, 4, 1], [0, 0, 8, 14], 3)
            # cap below the count: the first row only
            a[:], s[:], f[:] = 0xA5, 0xA5, 0xA5
            assert form(0, 6, 1, a, s, f, count) == OK and count.value == 2
            assert a[0].tolist() == [4, 4, 4, 0] and (a[1:] == 0xA5).all() and (f[1:] == 0xA5).all()
            a[:], s[:], f[:] = 0xA5, 0xA5, 0xA5
            count.value = 77
        assert b"not a range" in L.qp_ledger_last_error(h) or b"null" in L.qp_ledger_last_error(h)
        # the log-only form: null log buffers, n outside 1..2^31, a non-canonical account or flags > 1 in the range
        for kw in ({"acc": None}, {"amt": None}, {"fl": None}, {"n": 0}, {"n": 2**31 + 1}):
            assert log_form(0, 1, 3, a, s, f, count, **kw) == ERR_ARG, kw
        bad = acc.copy()
        bad[2, 1] = P
        assert log_form(0, 6, 3, a, s, f, count, acc=bad) == ERR_ARG
        assert b"account of entry 2" in L.qp_ledger_last_error(None)
        assert log_form(3, 6, 3, a, s, f, count, acc=bad) == OK  # outside the range it is not read
        bad = fl.copy()
        bad[5] = 2
        assert log_form(0, 6, 3, a, s, f, count, fl=bad) == ERR_ARG and b"flags of entry 5" in L.qp_ledger_last_error(None)
        assert log_form(0, 5, 3, a, s, f, count, fl=bad) == OK
    finally:
        L.qp_ledger_free(h)
