"""The nullifier-set commitment on the host path (ctx=None): root, m, order and
every proof against the plain-Python model (nullifier_set_model.py) for a ballot
box and a transfer ledger; the checker's refusals for every single-word tamper;
duplicates; the commit's caching; the refusals of the new calls."""
import random
import re

import numpy as np
import pytest

import qp_wormhole
from nullifier_set_model import (NON_CANONICAL, NULL, OK, ORDER, ROOT, SHAPE, P, SetModel, as_tuple, cast_keys, handle_log,
                                 make_handle, model_check, model_tuple, pattern_keys, queries, random_keys)
from qp_wormhole.nullifier_set import NullifierLeaf, NullifierProof, nullifier_proof_status

KINDS = ["box", "ledger"]
HEADER = qp_wormhole._native.HEADER
SYMBOLS = {"qp_ballot_box_commit_set": 3, "qp_ledger_commit_set": 3, "qp_ballot_box_set_proofs": 17,
           "qp_ledger_set_proofs": 17, "qp_nullifier_set_root": 8, "qp_nullifier_set_check": 15,
           "qp_nullifier_set_tile": 0, "qp_nullifier_set_last_error": 0, "qp_nullifier_set_times": 2}


def test_symbols_declared_exported_and_bound():
    L = qp_wormhole.lib()
    declared = qp_wormhole.header_symbols()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s, arity in SYMBOLS.items():
        assert s in declared, s
        f = getattr(L, s)
        assert f.argtypes is not None and len(f.argtypes) == arity, s
        m = re.search(r"^[\w ]+?\*?%s\s*\(([^)]*)\)\s*;" % s, txt, re.M)
        args = m.group(1).strip()
        assert m and (0 if args == "void" else len(args.split(","))) == arity, s
    for name in ("NullifierProof", "NullifierLeaf", "check_nullifier_proof", "nullifier_set_root"):
        assert name in qp_wormhole.__all__ and hasattr(qp_wormhole, name)
    for cls in (qp_wormhole.BallotBox, qp_wormhole.WormholeLedger):
        for name in ("commit_nullifiers", "nullifier_proofs", "nullifier_proof_for", "check_nullifier_proof"):
            assert hasattr(cls, name)
    assert qp_wormhole.nullifier_set_tile() >= 64


def check_handle_against_model(kind, h, rng):
    model = SetModel(*handle_log(kind, h))
    assert h.commit_nullifiers() == (model.root, model.m)
    root, m, order, dup = qp_wormhole.nullifier_set_root(None, h.entries())
    assert (root, m, order, dup) == (model.root, model.m, model.order, None)
    q = queries(model, rng)
    proofs = h.nullifier_proofs(q)
    for x, p in zip(q, proofs):
        assert (p.key, p.root, p.m) == (x, model.root, model.m)
        assert as_tuple(p) == model_tuple(model.proof(x)), x
        assert nullifier_proof_status(p) == OK and h.check_nullifier_proof(p)
    return model, proofs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [0, 1, 2, 3, 300])
def test_root_order_and_proofs_match_model(kind, m):
    rng = random.Random(f"sizes {kind} {m}")
    h = make_handle(kind, None, max(m, 1) + 8)
    try:
        keys = random_keys(rng, m)
        if keys:
            # non-members interleaved: every third key is cast twice, the second a double
            stream = [k for i, k in enumerate(keys) for k in ([k, keys[i // 2]] if i % 3 == 2 else [k])]
            h.reserve(len(stream))
            cast_keys(kind, h, stream)
        model, _ = check_handle_against_model(kind, h, rng)
        assert model.m == m
    finally:
        h.free()


@pytest.mark.parametrize("name", ["felt3_only", "high32_only", "low32_only", "edges"])
def test_key_patterns(name):
    rng = random.Random("patterns " + name)
    h = make_handle("ledger", None, 64)
    try:
        cast_keys("ledger", h, pattern_keys(name, 37))
        check_handle_against_model("ledger", h, rng)
    finally:
        h.free()


def tampers(p):
    """every single-word tamper of proof p: (what, tampered proof, root, m)"""
    out = []

    def slot(which, **kw):
        return p._replace(**{which: getattr(p, which)._replace(**kw)})

    def bump(v, i):
        v = list(v)
        v[i] ^= 1
        return v

    for i in range(4):
        out.append((f"key[{i}]", p._replace(key=bump(p.key, i)), p.root, p.m))
        out.append((f"root[{i}]", p, bump(p.root, i), p.m))
    far = list(p.key)
    far[0] ^= 1 << 62  # a key far from x: outside the two leaves
    out.append(("key far", p._replace(key=far), p.root, p.m))
    for which in ("lo", "hi"):
        s = getattr(p, which)
        if s is None:
            continue
        for i in range(4):
            out.append((f"{which}.key[{i}]", slot(which, key=bump(s.key, i)), p.root, p.m))
        out.append((f"{which}.seq", slot(which, seq=s.seq ^ 1), p.root, p.m))
        for d in range(s.depth):
            for i in range(4):
                sib = [list(x) for x in s.siblings]
                sib[d][i] ^= 1
                out.append((f"{which}.sib[{d}][{i}]", slot(which, siblings=sib), p.root, p.m))
        for b in range(max(s.depth, 1)):
            out.append((f"{which}.bits^{1 << b}", slot(which, path_bits=s.path_bits ^ (1 << b)), p.root, p.m))
        out.append((f"{which}.depth-1", slot(which, depth=s.depth - 1, siblings=s.siblings[:-1]), p.root, p.m))
    out.append(("found", p._replace(found=not p.found), p.root, p.m))
    for d in (-1, 1):
        if 0 <= p.pos + d:
            out.append((f"pos{d:+d}", p._replace(pos=p.pos + d), p.root, p.m))
        if 0 <= p.m + d:
            out.append((f"m{d:+d}", p, p.root, p.m + d))
    return out


def test_checker_refuses_every_single_word_tamper():
    rng = random.Random("tamper")
    h = make_handle("box", None, 64)
    try:
        keys = sorted(random_keys(rng, 21))
        cast_keys("box", h, rng.sample(keys, len(keys)))
        # m = 21 is odd and the two proofs end at the last leaf, so m - 1 and m + 1 both change a leaf's
        # shape.  The checker binds m through the shape alone, as a receipt binds n: (root, m) is what
        # the operator publishes and is never taken from the proof.  The "mid" proofs show the other
        # side: a leaf whose shape is the same under m - 1 still checks there.
        absent = keys[19][:3] + [keys[19][3] + 1]
        mid = keys[9][:3] + [keys[9][3] + 1]
        cases = {"absence": h.nullifier_proof_for(absent), "membership": h.nullifier_proof_for(keys[20]),
                 "mid absence": h.nullifier_proof_for(mid), "mid membership": h.nullifier_proof_for(keys[12]),
                 "below all": h.nullifier_proof_for([0, 0, 0, 0]), "above all": h.nullifier_proof_for([P - 1] * 4)}
        assert (cases["absence"].found, cases["absence"].pos, cases["membership"].pos) == (False, 20, 20)
        seen = set()
        for name, p in cases.items():
            assert nullifier_proof_status(p) == OK
            for what, t, root, m in tampers(p):
                want = model_check(t.key, t.found, t.pos, t.lo, t.hi, root, m)
                got = nullifier_proof_status(t, root, m)
                assert got == want, (name, what, got, want)
                # an absence proof holds for every key between its two leaves, so a key moved inside
                # them is another valid proof; every other tamper is refused
                assert got != OK or (not p.found and what.startswith("key[")) or \
                    (name not in ("absence", "membership") and what in ("m-1", "m+1")), (name, what)
                assert h.check_nullifier_proof(t, root, m) == (got == OK)
                seen.add(got)
        assert seen >= {OK, SHAPE, ROOT, ORDER}
        # a felt >= p anywhere is non-canonical before anything else
        p = cases["absence"]
        for t in (p._replace(key=p.key[:3] + [P]), p._replace(lo=p.lo._replace(seq=P)),
                  p._replace(hi=p.hi._replace(siblings=[[P, 0, 0, 0]] + p.hi.siblings[1:]))):
            assert nullifier_proof_status(t) == NON_CANONICAL
        assert nullifier_proof_status(p, root=[P, 0, 0, 0]) == NON_CANONICAL
        z = np.zeros(128, np.uint64)
        assert qp_wormhole.lib().qp_nullifier_set_check(None, 1, z.ctypes.data, 0, 0, z.ctypes.data, 0, z.ctypes.data, 0, 0,
                                                        z.ctypes.data, 0, z.ctypes.data, 0, 0) == NULL
    finally:
        h.free()


def test_no_absence_proof_for_a_member_from_honest_leaves():
    """x is in the set at position j.  An absence proof would need adjacent leaves around x: the
    honest leaves at (j - 1, j) or (j, j + 1), offered with pos = j or j + 1, fail the order test, and
    the leaves (j - 1, j + 1) are not adjacent, so no pos gives both their shapes and roots."""
    rng = random.Random("member absence")
    h = make_handle("ledger", None, 64)
    try:
        keys = sorted(random_keys(rng, 16))
        cast_keys("ledger", h, keys)
        model = SetModel(*handle_log("ledger", h))
        j = 6
        x = keys[j]
        leaf = lambda i: NullifierLeaf(*model.leaf(i))  # noqa: E731
        for pos, lo, hi in ((j, leaf(j - 1), leaf(j)), (j + 1, leaf(j), leaf(j + 1)), (j, leaf(j - 1), leaf(j + 1)),
                            (j + 1, leaf(j - 1), leaf(j + 1))):
            t = NullifierProof(x, False, pos, lo, hi, model.root, model.m)
            got = nullifier_proof_status(t)
            assert got != OK and got == model_check(x, False, pos, tuple(lo), tuple(hi), model.root, model.m)
        p = h.nullifier_proof_for(x)
        assert p.found and nullifier_proof_status(p) == OK
        for d in (-1, 1):
            assert nullifier_proof_status(p._replace(pos=p.pos + d)) != OK
    finally:
        h.free()


@pytest.mark.parametrize("kind", KINDS)
def test_commit_caching_staleness_and_the_log_commitment(kind):
    rng = random.Random("stale " + kind)
    h = make_handle(kind, None, 64)
    try:
        keys = random_keys(rng, 12)
        cast_keys(kind, h, keys[:8])
        log0 = h.commit_log()
        c0 = h.commit_nullifiers()
        assert h.commit_nullifiers() == c0 and h.commit_log() == log0  # idempotent; the log root is untouched
        absent = h.nullifier_proof_for(keys[9])
        assert not absent.found and h.check_nullifier_proof(absent)
        statuses = cast_keys(kind, h, keys[:4])  # all doubles: admitted to the log, nothing new in the set
        assert all(s == 6 for s in statuses)
        c1 = h.commit_nullifiers()
        assert c1 == c0 and h.check_nullifier_proof(absent, *c1)
        log1 = h.commit_log()
        assert log1[1] == 12 and log1 != log0
        cast_keys(kind, h, keys[8:])  # admits keys[9]
        c2 = h.commit_nullifiers()
        assert c2[1] == 12 and c2 != c1
        assert not h.check_nullifier_proof(absent, *c2)  # a proof under a stale (root, m) fails
        assert h.nullifier_proof_for(keys[9]).found
        assert h.commit_log()[1] == 16
        model = SetModel(*handle_log(kind, h))
        assert c2 == (model.root, model.m) and sum(handle_log(kind, h)[1]) == 12
    finally:
        h.free()


@pytest.mark.parametrize("kind", KINDS)
def test_restored_handle_and_reserve(kind):
    rng = random.Random("restore " + kind)
    h = make_handle(kind, None, 64)
    try:
        keys = random_keys(rng, 20)
        cast_keys(kind, h, keys + keys[:5])
        want = h.commit_nullifiers()
        if kind == "box":
            r = qp_wormhole.BallotBox.restore(None, [0x2A2A2A2A2A2A2A2A] * 4, [[11, 12, 13, P - 1]], h.entries())
        else:
            r = qp_wormhole.WormholeLedger.restore(None, [[11, 12, 13, P - 1]], h.entries())
        try:
            assert r.commit_nullifiers() == want
            r.reserve(4096)
            assert r.commit_nullifiers() == want
            assert [as_tuple(p) for p in r.nullifier_proofs(keys[:3])] == [as_tuple(p) for p in h.nullifier_proofs(keys[:3])]
        finally:
            r.free()
    finally:
        h.free()


def test_duplicate_members_in_a_published_log():
    rng = random.Random("dups")
    keys = random_keys(rng, 40)
    nul = keys + [keys[7], keys[30], keys[7]]  # seqs 40, 41, 42 repeat members 7, 30, 7
    member = [1] * len(nul)
    model = SetModel(nul, member)
    assert model.duplicate == 40
    assert qp_wormhole.nullifier_set_root(None, (nul, member)) == (model.root, model.m, model.order, 40)
    member[40] = 0  # not a member: the lowest offender is now 41
    model = SetModel(nul, member)
    assert qp_wormhole.nullifier_set_root(None, (nul, member)) == (model.root, model.m, model.order, 41)
    member[41] = member[42] = 0
    assert qp_wormhole.nullifier_set_root(None, (nul, member))[3] is None
    with pytest.raises(qp_wormhole.QpError, match="member entry 3 is not four canonical"):
        qp_wormhole.nullifier_set_root(None, (keys[:3] + [[P, 0, 0, 0]], [1, 1, 1, 1]))
    assert qp_wormhole.nullifier_set_root(None, (keys[:3] + [[P, 0, 0, 0]], [1, 1, 1, 0]))[1] == 3


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    L = qp_wormhole.lib()
    abi = "qp_ballot_box" if kind == "box" else "qp_ledger"
    h = make_handle(kind, None, 8)
    try:
        commit, proofs, last = getattr(L, abi + "_commit_set"), getattr(L, abi + "_set_proofs"), getattr(L, abi + "_last_error")
        assert commit(None, None, None) == 1  # QP_ERR_ARG: no handle
        assert commit(h.h, None, None) == 0
        k = np.array([[1, 2, 3, 4]], np.uint64)
        nulls = [None] * 12
        assert proofs(h.h, k.ctypes.data, 1, *nulls, None, None) == 1
        assert last(h.h).decode() == abi + "_set_proofs: null buffer"
        assert proofs(h.h, None, 0, *nulls, None, None) == 0
        with pytest.raises(qp_wormhole.QpError, match=abi + "_set_proofs: nullifier at position 1 felt 2 is not a canonical"):
            h.nullifier_proofs(np.array([[1, 2, 3, 4], [1, 2, P, 4]], np.uint64))
    finally:
        h.free()
