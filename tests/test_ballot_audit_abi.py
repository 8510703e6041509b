"""CPU-side checks of the audit part of the C ABI through ctypes on the host
path: the entry points are declared, exported and bound with the header's
arity; null pointers and n = 0 are refused; roots_at names a size outside
1..admitted by its position; k = 0 is accepted; an empty log is QP_ERR_STATE."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")
P = 0xFFFFFFFF00000001
PROPOSAL = np.array([1, 2, 3, 4], np.uint64)
ROOT = np.array([5, 6, 7, 8], np.uint64)
NONE = 2**64 - 1

SYMBOLS = {"qp_ballot_log_audit": 11, "qp_ballot_box_roots_at": 4, "qp_ballot_box_restore": 12}


def test_symbols_declared_exported_and_bound():
    L = qp_wormhole.lib()
    declared = qp_wormhole.header_symbols()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s, arity in SYMBOLS.items():
        assert s in declared, s
        f = getattr(L, s)
        assert f.argtypes is not None and len(f.argtypes) == arity, s
        m = re.search(r"^[\w ]+?\*?%s\s*\(([^)]*)\)\s*;" % s, txt, re.M)
        assert m and len(m.group(1).split(",")) == arity, s
    enum = re.search(r"typedef enum \{([^}]*)\} qp_audit_status;", txt, re.S).group(1)
    assert re.findall(r"QP_AUDIT_(\w+) = (\d+)", enum) == [("OK", "0"), ("NON_CANONICAL", "1"), ("ORDER", "2"),
                                                           ("COUNT_RULE", "3"), ("TALLY", "4"), ("ROOT", "5"),
                                                           ("COMMITMENT", "6")]
    assert qp_wormhole.ballot.AUDIT_DTYPE.itemsize == 80


def box_with(n, capacity=8):
    L = qp_wormhole.lib()
    h = ctypes.c_void_p()
    assert L.qp_ballot_box_new(None, PROPOSAL, ROOT, 1, capacity, ctypes.byref(h)) == 0
    if n:
        pis = np.array([list(PROPOSAL) + list(ROOT) + [i & 1, 9, 9, 9, i] for i in range(n)], np.uint64)
        res = np.zeros(n, qp_wormhole.ballot.RESULT_DTYPE)
        assert L.qp_ballot_box_cast_public(h, pis.ctypes.data, None, n, res.ctypes.data) == 0
    return L, h


def published(L, h, n):
    nul, num, fl = np.zeros((n, 4), np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    assert L.qp_ballot_box_entries(h, 0, n, nul.ctypes.data, num.ctypes.data, fl.ctypes.data) == 0
    return nul, num, fl


def test_audit_arguments():
    L, h = box_with(5)
    try:
        nul, num, fl = published(L, h, 5)
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        assert L.qp_ballot_box_commit_log(h, root.ctypes.data, ctypes.byref(n)) == 0
    finally:
        L.qp_ballot_box_free(h)
    rep = np.zeros(1, qp_wormhole.ballot.AUDIT_DTYPE)
    tally = np.array([2, 3], np.uint64)
    cns = np.array([5], np.uint64)

    def audit(nul=nul, num=num, fl=fl, n=5, root=root, tally=tally, croots=root, cns=cns, ncommit=1, out=rep):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.qp_ballot_log_audit(None, p(nul), p(num), p(fl), n, p(root), p(tally), p(croots), p(cns), ncommit, p(out))
    assert audit() == 0
    r = rep[0]
    assert (int(r["status"]), int(r["witness"]), int(r["first"])) == (0, NONE, NONE)
    assert (r["root"].tolist(), int(r["yes"]), int(r["no"]), int(r["counted"])) == (root.tolist(), 2, 3, 5)
    # every claim is optional
    assert audit(root=None, tally=None, croots=None, cns=None, ncommit=0) == 0 and int(rep[0]["status"]) == 0
    # null pointers, n = 0, n above 2^31
    assert audit(out=None) == 1
    for name in ("nul", "num", "fl"):
        assert audit(**{name: None}) == 1, name
        assert b"qp_ballot_log_audit: null buffer" in L.qp_ballot_box_last_error(None)
    assert audit(croots=None) == 1 and audit(cns=None) == 1
    assert audit(n=0) == 1 and b"0 entries" in L.qp_ballot_box_last_error(None)
    assert audit(n=2**31 + 1) == 1
    # n_i == 0 and a non-canonical claimed root are refusals, not audit results
    assert audit(cns=np.array([0], np.uint64)) == 1 and b"commitment 0 names n = 0" in L.qp_ballot_box_last_error(None)
    bad = root.copy()
    bad[2] = P
    assert audit(root=bad) == 1 and b"claimed root" in L.qp_ballot_box_last_error(None)
    assert audit(croots=bad) == 1 and b"commitment 0" in L.qp_ballot_box_last_error(None)
    # the verdict is in the report, the return value stays QP_OK
    assert audit(tally=np.array([3, 2], np.uint64)) == 0 and int(rep[0]["status"]) == 4
    assert audit(cns=np.array([6], np.uint64)) == 0
    assert (int(rep[0]["status"]), int(rep[0]["witness"])) == (6, 0)


def test_roots_at_arguments():
    L, h = box_with(3)
    try:
        out = np.full((2, 4), 7, np.uint64)
        root = np.zeros(4, np.uint64)
        ms = np.array([3, 1], np.uint64)
        assert L.qp_ballot_box_roots_at(None, ms.ctypes.data, 2, out.ctypes.data) == 1
        assert L.qp_ballot_box_roots_at(h, None, 2, out.ctypes.data) == 1
        assert L.qp_ballot_box_roots_at(h, ms.ctypes.data, 2, None) == 1
        assert b"null buffer" in L.qp_ballot_box_last_error(h)
        # k == 0 is QP_OK whatever the pointers, and writes nothing
        assert L.qp_ballot_box_roots_at(h, None, 0, None) == 0 and (out == 7).all()
        assert L.qp_ballot_box_roots_at(h, ms.ctypes.data, 2, out.ctypes.data) == 0
        assert L.qp_ballot_box_commit_log(h, root.ctypes.data, None) == 0
        assert out[0].tolist() == root.tolist() and out[1].tolist() != root.tolist()
        # a size outside 1..admitted, named by its position
        for bad, pos in (([3, 0], 1), ([4, 1], 0), ([1, 2**40], 1)):
            ms[:] = bad
            assert L.qp_ballot_box_roots_at(h, ms.ctypes.data, 2, out.ctypes.data) == 1
            assert b"position %d" % pos in L.qp_ballot_box_last_error(h)
    finally:
        L.qp_ballot_box_free(h)
    L, h = box_with(0)
    try:
        assert L.qp_ballot_box_roots_at(h, None, 0, None) == 4
        assert b"empty log" in L.qp_ballot_box_last_error(h)
    finally:
        L.qp_ballot_box_free(h)


def test_restore_arguments():
    L, h = box_with(5)
    try:
        nul, num, fl = published(L, h, 5)
    finally:
        L.qp_ballot_box_free(h)
    out = ctypes.c_void_p()

    def restore(nul=nul, num=num, fl=fl, n=5, capacity=8, cast_count=5, expect=None, proposal=PROPOSAL):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.qp_ballot_box_restore(None, proposal, ROOT, 1, capacity, p(nul), p(num), p(fl), n, cast_count,
                                       p(expect), ctypes.byref(out))
    assert restore() == 0 and out.value
    cast, adm, cap = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    assert L.qp_ballot_box_state(out, ctypes.byref(cast), ctypes.byref(adm), ctypes.byref(cap)) == 0
    assert (cast.value, adm.value, cap.value) == (5, 5, 8)
    L.qp_ballot_box_free(out)
    for name in ("nul", "num", "fl"):
        assert restore(**{name: None}) == 1 and not out.value, name
    assert restore(nul=None, num=None, fl=None, n=0, cast_count=0) == 0 and out.value  # an empty log needs no buffers
    L.qp_ballot_box_free(out)
    assert restore(capacity=4) == 1 and b"capacity" in L.qp_ballot_box_last_error(None)
    assert restore(cast_count=4) == 1 and b"cast_count" in L.qp_ballot_box_last_error(None)
    assert restore(proposal=np.array([P, 0, 0, 0], np.uint64)) == 1  # qp_ballot_box_new's own refusals
    assert restore(expect=np.array([P, 0, 0, 0], np.uint64)) == 1
    assert restore(expect=ROOT) == 6 and b"claimed root differs" in L.qp_ballot_box_last_error(None) and not out.value
    bad = fl.copy()
    bad[3] = 1
    assert restore(fl=bad) == 6 and b"count rule" in L.qp_ballot_box_last_error(None)
    assert b"entry 3" in L.qp_ballot_box_last_error(None)
