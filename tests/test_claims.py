"""Payout claims on the host path (ctx=None): root, count, total, order and every
claim against the plain-Python model (claims_model.py); carries across every
limb boundary; ranges with m0 > 0; the checker's refusals for every single-word
tamper; rounds that add up; the auditor's form; the refusals of the new calls;
the ledger's other answers unchanged."""
import random
import re

import numpy as np
import pytest

import qp_wormhole
from claims_model import (MAX_AMOUNT, NON_CANONICAL, NULL, OK, ORDER, PATTERNS, ROOT, SHAPE, ClaimsModel, P, Stream,
                          as_tuple, cast, mixed_stream, model_check, model_of, model_tuple, new_ledger,
                          pattern_accounts, queries, random_accounts)
from qp_wormhole.claims import ClaimLeaf, PayoutClaim, check_claim_status

HEADER = qp_wormhole._native.HEADER
SYMBOLS = {"qp_ledger_commit_claims": 6, "qp_ledger_claims": 21, "qp_ledger_log_claims_root": 11,
           "qp_ledger_claim_check": 17, "qp_ledger_claims_times": 2}


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
    for name in ("PayoutClaim", "ClaimLeaf", "ClaimsCommitment", "check_claim", "check_claim_status",
                 "ledger_log_claims_root", "claims_times"):
        assert name in qp_wormhole.__all__ and hasattr(qp_wormhole, name)
    for name in ("commit_claims", "claims", "claim_for", "check_claim"):
        assert hasattr(qp_wormhole.WormholeLedger, name)


def check_range_against_model(led, m0, m1, rng, extra=()):
    """commitment, auditor's form and the claims of `queries` for [m0, m1) against the model"""
    model = model_of(led, m0, m1)
    c = led.commit_claims(m0, m1)
    assert tuple(c) == (model.root, model.count, model.total, m0, led.admitted if m1 is None else m1)
    assert led.commit_claims(m0, m1) == c  # the same range twice: the same triple
    if led.admitted:
        assert qp_wormhole.ledger_log_claims_root(None, led.entries(), m0, m1) == (model.root, model.count, model.total,
                                                                                     model.order)
    else:  # nothing was published: the log form refuses what the log payouts refuse
        with pytest.raises(qp_wormhole.QpError, match="a log of 0 entries: a published log has 1 to 2\\^31"):
            qp_wormhole.ledger_log_claims_root(None, led.entries(), m0, m1)
    q = queries(model, rng) + [list(x) for x in extra]
    claims = led.claims(q, m0, m1)
    for x, p in zip(q, claims):
        assert (p.account, p.root, p.count, p.m0, p.m1) == (x, model.root, model.count, c.m0, c.m1)
        assert as_tuple(p) == model_tuple(model.claim(x)), x
        assert check_claim_status(p) == OK and qp_wormhole.check_claim(p, c.root, c.count)
        assert p.total == (model.totals[p.pos] if p.found else 0)
    return model, claims


@pytest.mark.parametrize("A", [0, 1, 2, 3, 300])
def test_commitment_and_claims_match_model(A):
    rng = random.Random(f"claims sizes {A}")
    accounts = random_accounts(rng, A)
    s = mixed_stream(A, accounts) if A else Stream(A)
    led = new_ledger(None, len(s.rows) + 8)
    try:
        cast(led, s)
        model, _ = check_range_against_model(led, 0, None, rng)
        assert model.count == A
        if A:
            assert sum(1 for c in led.entries()[4] if not c) > 0 or A < 3  # double spends sit in the log
            assert led.admitted < len(s.rows) or A < 4                      # the unknown roots do not
    finally:
        led.free()


def test_range_of_double_spends_only_is_empty():
    rng = random.Random("claims doubles")
    s = Stream("doubles")
    accounts = random_accounts(rng, 5)
    for a in accounts:
        s.credit(a, 100)
    for a in accounts + accounts:
        s.double(a)
    led = new_ledger(None, 32)
    try:
        cast(led, s)
        assert led.admitted == 15
        model, claims = check_range_against_model(led, 5, 15, rng, extra=accounts)
        assert (model.count, model.root, model.total) == (0, [0, 0, 0, 0], 0)
        assert all(as_tuple(p) == (False, 0, None, None) for p in claims)
        # m0 == m1: the empty commitment, anywhere in the log
        for m in (0, 7, 15):
            assert tuple(led.commit_claims(m, m)) == ([0, 0, 0, 0], 0, 0, m, m)
    finally:
        led.free()


def test_range_with_accounts_credited_before_and_inside():
    """m0 > 0: an account credited before the range and again inside appears with its in-range total
    and its in-range first_seq; one credited only before is absent"""
    rng = random.Random("claims m0")
    accounts = random_accounts(rng, 12)
    s = Stream("m0")
    for a in accounts[:8]:
        s.credit(a, rng.randrange(1 << 100))
    s.double(accounts[0])
    m0 = len(s.rows)
    for a in accounts[4:]:
        s.credit(a, rng.randrange(1 << 128))
        s.double(accounts[1])
    for a in accounts[6:10]:
        s.credit(a, rng.randrange(1 << 128))
    led = new_ledger(None, 64)
    try:
        cast(led, s)
        model, claims = check_range_against_model(led, m0, None, rng, extra=accounts)
        assert model.count == 8 and min(model.order) >= m0
        by_account = {tuple(p.account): p for p in claims}
        assert not by_account[tuple(accounts[0])].found
        inside = by_account[tuple(accounts[4])]
        assert inside.found and inside.hi.first_seq >= m0 and inside.total < led.total_for(accounts[4])
        check_range_against_model(led, 3, m0 + 5, rng)
    finally:
        led.free()


def test_carries_cross_every_limb_boundary():
    """an account whose entries all have every amount limb 0xFFFFFFFF: with three entries each limb
    sum is 3 (2^32 - 1) and a carry crosses every boundary up into limb 0 of the five; one with
    all-zero amounts; one whose sums stay below 2^32"""
    rng = random.Random("claims carries")
    full, zero, small = random_accounts(rng, 3)
    s = Stream("carries")
    for _ in range(3):
        s.credit(full, MAX_AMOUNT)
        s.credit(zero, 0)
        s.credit(small, 5)
    led = new_ledger(None, 16)
    try:
        cast(led, s)
        model, claims = check_range_against_model(led, 0, None, rng)
        by_account = {tuple(p.account): p for p in claims if p.found}
        assert by_account[tuple(full)].total == 3 * MAX_AMOUNT >= 1 << 128
        assert by_account[tuple(zero)].total == 0 and by_account[tuple(zero)].found
        assert by_account[tuple(small)].total == 15
        assert model.total == 3 * MAX_AMOUNT + 15 == led.recount()[2]
    finally:
        led.free()


@pytest.mark.parametrize("name", PATTERNS)
def test_key_patterns(name):
    rng = random.Random("claims patterns " + name)
    led = new_ledger(None, 128)
    try:
        cast(led, mixed_stream(name, pattern_accounts(name, 37)))
        check_range_against_model(led, 0, None, rng)
    finally:
        led.free()


def tampers(p):
    """every single-word tamper of claim p: (what, tampered claim, root, count)"""
    out = []

    def slot(which, **kw):
        return p._replace(**{which: getattr(p, which)._replace(**kw)})

    def bump(v, i):
        v = list(v)
        v[i] ^= 1
        return v

    for i in range(4):
        out.append((f"account[{i}]", p._replace(account=bump(p.account, i)), p.root, p.count))
        out.append((f"root[{i}]", p, bump(p.root, i), p.count))
    far = list(p.account)
    far[0] ^= 1 << 62  # an account far from x: outside the two leaves
    out.append(("account far", p._replace(account=far), p.root, p.count))
    for which in ("lo", "hi"):
        s = getattr(p, which)
        if s is None:
            continue
        for i in range(4):
            out.append((f"{which}.account[{i}]", slot(which, account=bump(s.account, i)), p.root, p.count))
        for i in range(5):
            out.append((f"{which}.total limb {i}", slot(which, total=s.total ^ (1 << (128 - 32 * i))), p.root, p.count))
        out.append((f"{which}.first_seq", slot(which, first_seq=s.first_seq ^ 1), p.root, p.count))
        for d in range(s.depth):
            for i in range(4):
                sib = [list(x) for x in s.siblings]
                sib[d][i] ^= 1
                out.append((f"{which}.sib[{d}][{i}]", slot(which, siblings=sib), p.root, p.count))
        for b in range(max(s.depth, 1)):
            out.append((f"{which}.bits^{1 << b}", slot(which, path_bits=s.path_bits ^ (1 << b)), p.root, p.count))
        out.append((f"{which}.depth-1", slot(which, depth=s.depth - 1, siblings=s.siblings[:-1]), p.root, p.count))
    out.append(("found", p._replace(found=not p.found), p.root, p.count))
    for d in (-1, 1):
        if 0 <= p.pos + d:
            out.append((f"pos{d:+d}", p._replace(pos=p.pos + d), p.root, p.count))
        if 0 <= p.count + d:
            out.append((f"count{d:+d}", p, p.root, p.count + d))
    return out


def test_checker_refuses_every_single_word_tamper():
    rng = random.Random("claims tamper")
    accounts = sorted(random_accounts(rng, 21))
    s = Stream("tamper")
    for a in rng.sample(accounts, len(accounts)):
        s.credit(a, rng.randrange(1 << 128))
    led = new_ledger(None, 64)
    try:
        cast(led, s)
        # A = 21 is odd and the first two claims end at the last leaf, so A - 1 and A + 1 both change a
        # leaf's shape: A is bound through the shape alone.  The "mid" claims show the other side: a
        # leaf whose shape is the same under A - 1 still checks there.
        absent = accounts[19][:3] + [accounts[19][3] + 1]
        mid = accounts[9][:3] + [accounts[9][3] + 1]
        cases = {"absence": led.claim_for(absent), "membership": led.claim_for(accounts[20]),
                 "mid absence": led.claim_for(mid), "mid membership": led.claim_for(accounts[12]),
                 "below all": led.claim_for([0, 0, 0, 0]), "above all": led.claim_for([P - 1] * 4)}
        assert (cases["absence"].found, cases["absence"].pos, cases["membership"].pos) == (False, 20, 20)
        seen = set()
        for name, p in cases.items():
            assert check_claim_status(p) == OK
            for what, t, root, count in tampers(p):
                want = model_check(t.account, t.found, t.pos, t.lo, t.hi, root, count)
                got = check_claim_status(t, root, count)
                assert got == want, (name, what, got, want)
                # an absence claim holds for every account between its two leaves, so an account moved
                # inside them is another valid claim; every other tamper is refused
                assert got != OK or (not p.found and what.startswith("account[")) or \
                    (name not in ("absence", "membership") and what in ("count-1", "count+1")), (name, what)
                assert qp_wormhole.check_claim(t, root, count) == (got == OK)
                seen.add(got)
        assert seen >= {OK, SHAPE, ROOT, ORDER}
        # a felt >= p anywhere is non-canonical before anything else
        p = cases["absence"]
        for t in (p._replace(account=p.account[:3] + [P]), p._replace(lo=p.lo._replace(first_seq=P)),
                  p._replace(hi=p.hi._replace(account=[P, 0, 0, 0])),
                  p._replace(hi=p.hi._replace(siblings=[[P, 0, 0, 0]] + p.hi.siblings[1:]))):
            assert check_claim_status(t) == NON_CANONICAL
        assert check_claim_status(p, root=[P, 0, 0, 0]) == NON_CANONICAL
        # a total that fits no five limbs is no claim
        assert not qp_wormhole.check_claim(p._replace(hi=p.hi._replace(total=1 << 160)))
        z = np.zeros(128, np.uint64)
        assert qp_wormhole.lib().qp_ledger_claim_check(None, 1, z.ctypes.data, 0, 0, z.ctypes.data, z.ctypes.data, 0,
                                                       z.ctypes.data, 0, 0, z.ctypes.data, z.ctypes.data, 0,
                                                       z.ctypes.data, 0, 0) == NULL
    finally:
        led.free()


def test_no_absence_claim_for_a_member_from_honest_leaves():
    """x is a row at position j.  An absence claim would need adjacent leaves around x: the honest
    leaves at (j - 1, j) or (j, j + 1), offered with pos = j or j + 1, fail the order test, and the
    leaves (j - 1, j + 1) are not adjacent, so no pos gives both their shapes and roots."""
    rng = random.Random("claims member absence")
    accounts = sorted(random_accounts(rng, 16))
    s = Stream("member absence")
    for a in accounts:
        s.credit(a, rng.randrange(1 << 128))
    led = new_ledger(None, 64)
    try:
        cast(led, s)
        model = model_of(led)
        j = 6
        x = accounts[j]
        leaf = lambda i: ClaimLeaf(*model.leaf(i))  # noqa: E731
        for pos, lo, hi in ((j, leaf(j - 1), leaf(j)), (j + 1, leaf(j), leaf(j + 1)), (j, leaf(j - 1), leaf(j + 1)),
                            (j + 1, leaf(j - 1), leaf(j + 1))):
            t = PayoutClaim(x, False, pos, lo, hi, model.root, model.count, 0, led.admitted)
            got = check_claim_status(t)
            assert got != OK and got == model_check(x, False, pos, tuple(lo), tuple(hi), model.root, model.count)
        p = led.claim_for(x)
        assert p.found and check_claim_status(p) == OK
        for d in (-1, 1):
            assert check_claim_status(p._replace(pos=p.pos + d)) != OK
    finally:
        led.free()


def test_rounds_add_up_and_other_answers_stand():
    """the found totals of consecutive rounds add up to the cumulative total account by account; the
    cumulative commitment's total is recount()'s; a claim of one range fails under another range's
    root; payouts, payouts_between, commit_log and commit_nullifiers answer as before"""
    rng = random.Random("claims rounds")
    accounts = random_accounts(rng, 40)
    s = mixed_stream("rounds", accounts)
    led = new_ledger(None, len(s.rows))
    try:
        cast(led, s)
        n = led.admitted
        a, b = n // 3, 2 * n // 3
        before = (led.payouts(), led.payouts_between(a, b), led.commit_log(), led.commit_nullifiers(), led.recount())
        whole = led.commit_claims()
        assert whole.total == led.recount()[2] and (whole.m0, whole.m1) == (0, n)
        cumulative = {tuple(p.account): p.total for p in led.claims(accounts)}
        rounds = [led.claims(accounts, m0, m1) for m0, m1 in ((0, a), (a, b), (b, n))]
        commitments = [led.commit_claims(m0, m1) for m0, m1 in ((0, a), (a, b), (b, n))]
        assert sum(c.total for c in commitments) == whole.total
        for i, acc in enumerate(accounts):
            assert sum(r[i].total for r in rounds) == cumulative[tuple(acc)] == led.total_for(acc)
        # a claim made under one range fails under another range's commitment
        p = next(p for p in rounds[1] if p.found)
        assert qp_wormhole.check_claim(p, commitments[1].root, commitments[1].count)
        for other in (commitments[0], commitments[2], whole):
            assert not qp_wormhole.check_claim(p, other.root, other.count)
        after = (led.payouts(), led.payouts_between(a, b), led.commit_log(), led.commit_nullifiers(), led.recount())
        assert after == before
        # a further cast: the range's commitment stands (the log is append-only), the open range moves on
        more = Stream("rounds more")
        more.credit(accounts[0], 11)
        cast(led, more)
        assert led.commit_claims(a, b) == commitments[1]
        assert led.commit_claims().total == whole.total + 11
        assert led.commit_claims(0, n) == whole
    finally:
        led.free()


def test_log_form_matches_the_ledger_and_refuses_a_bad_range():
    rng = random.Random("claims log")
    accounts = random_accounts(rng, 9)
    led = new_ledger(None, 64)
    try:
        cast(led, mixed_stream("log", accounts))
        n = led.admitted
        entries = led.entries()
        for m0, m1 in ((0, n), (2, n - 3), (5, 5)):
            c = led.commit_claims(m0, m1)
            root, count, total, order = qp_wormhole.ledger_log_claims_root(None, entries, m0, m1)
            assert (root, count, total) == (c.root, c.count, c.total) and len(order) == count
        nul, num, amt, acc, fl = entries
        with pytest.raises(qp_wormhole.QpError, match=r"qp_ledger_log_claims_root: entries \[4, 2\) are not a range"):
            qp_wormhole.ledger_log_claims_root(None, entries, 4, 2)
        with pytest.raises(qp_wormhole.QpError, match=r"entries \[0, %d\) are not a range of the log's %d" % (n + 1, n)):
            qp_wormhole.ledger_log_claims_root(None, entries, 0, n + 1)
        flags = np.asarray(fl).astype(np.uint8)
        flags[3] = 2
        with pytest.raises(qp_wormhole.QpError, match="the flags of entry 3 are above 1"):
            qp_wormhole.ledger_log_claims_root(None, (nul, num, amt, acc, flags))
        assert qp_wormhole.ledger_log_claims_root(None, (nul, num, amt, acc, flags), 4, n)[1] >= 1  # outside: not read
        bad = np.array(acc, dtype=np.uint64)
        bad[1, 2] = P
        with pytest.raises(qp_wormhole.QpError, match="the account of entry 1 is not four canonical"):
            qp_wormhole.ledger_log_claims_root(None, (nul, num, amt, bad, fl))
    finally:
        led.free()


def test_refusals():
    L = qp_wormhole.lib()
    led = new_ledger(None, 8)
    try:
        s = Stream("refusals")
        s.credit([1, 2, 3, 4], 5)
        s.credit([5, 6, 7, 8], 6)
        cast(led, s)
        assert L.qp_ledger_commit_claims(None, 0, 0, None, None, None) == 1  # QP_ERR_ARG: no ledger
        assert L.qp_ledger_commit_claims(led.h, 0, 2, None, None, None) == 0  # outputs may be null
        with pytest.raises(qp_wormhole.QpError, match=r"qp_ledger_commit_claims: entries \[2, 1\) are not a range"):
            led.commit_claims(2, 1)
        with pytest.raises(qp_wormhole.QpError, match=r"qp_ledger_commit_claims: entries \[0, 3\) are not a range of the log's 2"):
            led.commit_claims(0, 3)
        with pytest.raises(qp_wormhole.QpError, match=r"qp_ledger_claims: entries \[0, 3\) are not a range"):
            led.claims([[1, 2, 3, 4]], 0, 3)
        k = np.array([[1, 2, 3, 4]], np.uint64)
        nulls = [None] * 14
        assert L.qp_ledger_claims(led.h, 0, 2, k.ctypes.data, 1, *nulls, None, None) == 1
        assert L.qp_ledger_last_error(led.h).decode() == "qp_ledger_claims: null buffer"
        assert L.qp_ledger_claims(led.h, 0, 2, None, 0, *nulls, None, None) == 0  # k == 0: the commit alone
        with pytest.raises(qp_wormhole.QpError, match="qp_ledger_claims: account at position 1 felt 2 is not a canonical"):
            led.claims(np.array([[1, 2, 3, 4], [1, 2, P, 4]], np.uint64))
        assert qp_wormhole.claims_times() is None or isinstance(qp_wormhole.claims_times(), dict)
    finally:
        led.free()


def test_model_is_not_the_library():
    """the model's own pieces on a hand-made case: two accounts, a carry, the order by felt 0 first"""
    m = ClaimsModel([[2, 0, 0, 0], [1, 9, 9, 9], [2, 0, 0, 0]], [(1 << 128) - 1, 4, 1], [1, 1, 1])
    assert m.accounts == [[1, 9, 9, 9], [2, 0, 0, 0]] and m.totals == [4, 1 << 128] and m.order == [1, 0]
    assert m.claim([2, 0, 0, 0])[:2] == (True, 1) and m.claim([1, 9, 9, 10])[:2] == (False, 1)
    assert ROOT == 2
