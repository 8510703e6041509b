"""CPU-side checks of the log-commitment part of the C ABI through ctypes on the
host path: the entry points are declared, exported and bound with the header's
arity; null pointers are refused; k = 0 is accepted; qp_ballot_receipt_check
returns each reason code."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")
P = 0xFFFFFFFF00000001
PROPOSAL = np.array([1, 2, 3, 4], np.uint64)
ROOT = np.array([5, 6, 7, 8], np.uint64)
OK, SHAPE, ROOT_MISMATCH, NON_CANONICAL, NULL = range(5)

SYMBOLS = {"qp_ballot_box_find": 4, "qp_ballot_box_commit_log": 3, "qp_ballot_box_receipts": 9,
           "qp_ballot_box_entries_at": 6, "qp_ballot_receipt_check": 9}


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
    enum = re.search(r"typedef enum \{([^}]*)\} qp_receipt_status;", txt, re.S).group(1)
    assert re.findall(r"QP_RECEIPT_(\w+) = (\d+)", enum) == [("OK", "0"), ("SHAPE", "1"), ("ROOT", "2"),
                                                             ("NON_CANONICAL", "3"), ("NULL", "4")]


def box_with(n, capacity=8):
    L = qp_wormhole.lib()
    h = ctypes.c_void_p()
    assert L.qp_ballot_box_new(None, PROPOSAL, ROOT, 1, capacity, ctypes.byref(h)) == 0
    if n:
        pis = np.array([list(PROPOSAL) + list(ROOT) + [i & 1, 9, 9, 9, i] for i in range(n)], np.uint64)
        res = np.zeros(n, qp_wormhole.ballot.RESULT_DTYPE)
        assert L.qp_ballot_box_cast_public(h, pis.ctypes.data, None, n, res.ctypes.data) == 0
    return L, h


def test_null_pointers_and_k_zero():
    L, h = box_with(3)
    try:
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        q = np.array([[9, 9, 9, 1]], np.uint64)
        out = np.full(1, 7, np.uint64)
        sib = np.zeros((1, 32, 4), np.uint64)
        bits, depth = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        seqs = np.array([1], np.uint64)
        # null handles
        assert L.qp_ballot_box_find(None, q.ctypes.data, 1, out.ctypes.data) == 1
        assert L.qp_ballot_box_commit_log(None, root.ctypes.data, ctypes.byref(n)) == 1
        assert L.qp_ballot_box_receipts(None, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                        None, None, None) == 1
        assert L.qp_ballot_box_entries_at(None, seqs.ctypes.data, 1, None, None, None) == 1
        # null buffers with k > 0
        assert L.qp_ballot_box_find(h, None, 1, out.ctypes.data) == 1
        assert L.qp_ballot_box_find(h, q.ctypes.data, 1, None) == 1
        assert b"null buffer" in L.qp_ballot_box_last_error(h)
        assert L.qp_ballot_box_receipts(h, None, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data, None, None,
                                        None) == 1
        assert L.qp_ballot_box_receipts(h, seqs.ctypes.data, 1, None, bits.ctypes.data, depth.ctypes.data, None, None,
                                        None) == 1
        assert L.qp_ballot_box_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, None, depth.ctypes.data, None, None,
                                        None) == 1
        assert L.qp_ballot_box_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, None, None, None,
                                        None) == 1
        assert L.qp_ballot_box_entries_at(h, None, 1, None, None, None) == 1
        # k == 0 is QP_OK whatever the pointers; receipts still commits and reports the pair
        assert L.qp_ballot_box_find(h, None, 0, None) == 0 and out[0] == 7
        assert L.qp_ballot_box_entries_at(h, None, 0, None, None, None) == 0
        assert L.qp_ballot_box_receipts(h, None, 0, None, None, None, None, root.ctypes.data, ctypes.byref(n)) == 0
        assert n.value == 3 and root.any()
        # the optional outputs may be null
        assert L.qp_ballot_box_commit_log(h, None, None) == 0
        assert L.qp_ballot_box_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                        None, None, None) == 0
        assert (int(depth[0]), int(bits[0])) == (2, 1)  # entry 1 of 3: a right child, then a left one
        assert L.qp_ballot_box_find(h, q.ctypes.data, 1, out.ctypes.data) == 0 and out[0] == 1
        q[0, 3] = 5
        assert L.qp_ballot_box_find(h, q.ctypes.data, 1, out.ctypes.data) == 0 and out[0] == 2**64 - 1
        # an entry outside the log, and an empty box
        seqs[0] = 3
        assert L.qp_ballot_box_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                        None, None, None) == 1
        assert L.qp_ballot_box_entries_at(h, seqs.ctypes.data, 1, None, None, None) == 1
    finally:
        L.qp_ballot_box_free(h)
    L, h = box_with(0)
    try:
        assert L.qp_ballot_box_commit_log(h, None, None) == 4
        assert b"empty log" in L.qp_ballot_box_last_error(h)
        assert L.qp_ballot_box_receipts(h, None, 0, None, None, None, None, None, None) == 4
        assert L.qp_ballot_box_find(h, q.ctypes.data, 1, out.ctypes.data) == 0 and out[0] == 2**64 - 1
    finally:
        L.qp_ballot_box_free(h)


def test_receipt_check_reason_codes():
    L, h = box_with(5)
    try:
        root, n = np.zeros(4, np.uint64), ctypes.c_uint64()
        seqs = np.array([2], np.uint64)
        sib = np.zeros((32, 4), np.uint64)
        bits, depth = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        nul, num, fl = np.zeros(4, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint8)
        assert L.qp_ballot_box_receipts(h, seqs.ctypes.data, 1, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                        None, root.ctypes.data, ctypes.byref(n)) == 0
        assert L.qp_ballot_box_entries_at(h, seqs.ctypes.data, 1, nul.ctypes.data, num.ctypes.data, fl.ctypes.data) == 0
        assert (list(nul), int(num[0]), int(fl[0]), n.value) == ([9, 9, 9, 2], 2, 2, 5)
        d, b = int(depth[0]), int(bits[0])
        assert (d, b) == (3, 0b010)  # entry 2 of 5: left, right, left

        def check(root=root, n=5, seq=2, nul=nul, number=2, flags=2, sib=sib, bits=b, depth=d):
            return L.qp_ballot_receipt_check(None if root is None else root.ctypes.data, n, seq,
                                             None if nul is None else nul.ctypes.data, number, flags,
                                             None if sib is None else sib.ctypes.data, bits, depth)
        assert check() == OK
        assert check(root=None) == check(nul=None) == check(sib=None) == NULL
        # shape: seq and n, the depth, a side bit, a non-zero slot above the depth
        assert check(seq=5) == check(n=0) == check(n=2**31 + 1) == SHAPE
        assert check(depth=d - 1) == check(depth=d + 1) == check(depth=33) == check(bits=b ^ 2) == SHAPE
        assert check(n=4) == SHAPE  # four leaves give entry 2 a path of two
        dirty = sib.copy()
        dirty[d, 0] = 1
        assert check(sib=dirty) == SHAPE
        # root: the entry, a sibling, the root itself
        assert check(flags=3) == check(flags=0) == check(number=3) == ROOT_MISMATCH
        other = nul.copy()
        other[3] = 3
        wrong = sib.copy()
        wrong[0, 1] ^= 1
        assert check(nul=other) == check(sib=wrong) == check(root=ROOT) == ROOT_MISMATCH
        # a felt >= p, or a flags byte that is none of the log's
        for name in ("root", "nul", "sib"):
            bad = {"root": root, "nul": nul, "sib": sib}[name].copy()
            bad.reshape(-1)[1] = P
            assert check(**{name: bad}) == NON_CANONICAL, name
        assert check(number=P) == check(flags=4) == NON_CANONICAL
    finally:
        L.qp_ballot_box_free(h)
