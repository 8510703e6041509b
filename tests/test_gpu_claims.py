"""Payout claims on the device (the payout round's credit and compaction, the
nullifier set's tile sort, merge passes, search and gather over the account
column, csrc/claims.hip's leaves, grand total and totals gather, the levels and
paths through the accumulator tree's launchers): the device equals the host
path of the same library word for word (root, count, total, order and every
field of every claim), at the shapes where a sort, a merge or a batch changes
path, T = qp_nullifier_set_tile().  The host path is held to the plain-Python
model by test_claims.py."""
import numpy as np
import pytest

from claims_model import MAX_AMOUNT, PATTERNS, P, ROOT_A, amount_limbs, new_ledger, pattern_accounts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T():
    import qp_wormhole
    return qp_wormhole.nullifier_set_tile()


def rand_keys(seed, n):
    """n random canonical keys as a [n][4] uint64 array (distinct with overwhelming probability)"""
    return np.random.default_rng(seed).integers(0, P, size=(n, 4), dtype=np.uint64)


def transfers(nullifiers, accounts, amounts=None, seed=0):
    """pis [n][16]: one transfer per row under the accepted root; amounts [n][4] limbs (None: random)"""
    n = len(nullifiers)
    pis = np.zeros((n, 16), np.uint64)
    pis[:, 0:4] = nullifiers
    pis[:, 4:8] = ROOT_A
    pis[:, 8:12] = (np.random.default_rng(seed + 99).integers(0, 1 << 32, size=(n, 4), dtype=np.uint64)
                    if amounts is None else amounts)
    pis[:, 12:16] = accounts
    return pis


def stream_for(accounts, extra, seed):
    """credits for every account in a shuffled order; extra: some accounts credited again and double
    spends in between, so the range holds more entries than rows"""
    rng = np.random.default_rng(seed)
    A = len(accounts)
    acc = np.asarray(accounts, dtype=np.uint64).reshape(A, 4)
    order = rng.permutation(A)
    nul = rand_keys(seed + 1, A)
    pis = transfers(nul, acc[order], seed=seed)
    if not extra or not A:
        return pis
    again = rng.integers(0, A, A // 2 + 1)
    more = transfers(rand_keys(seed + 2, len(again)), acc[again], seed=seed + 3)
    cut = (A + 1) // 2  # the doubles spend nullifiers of the first `cut` credits and come after them
    doubles = transfers(nul[rng.integers(0, cut, A // 3 + 2)], acc[rng.integers(0, A, A // 3 + 2)], seed=seed + 4)
    tail = np.concatenate([more, doubles])
    tail = tail[rng.permutation(len(tail))]
    return np.concatenate([pis[:cut], tail[:len(tail) // 2], pis[cut:], tail[len(tail) // 2:]])


def pair(ctx, *batches):
    """a device ledger and a host ledger that were cast the same batches"""
    n = sum(len(b) for b in batches)
    dev, host = new_ledger(ctx, n), new_ledger(None, n)
    for h in (dev, host):
        for b in batches:
            if len(b):
                h.cast_public(b, raw=True)
    return dev, host


def sample_queries(host, m0, m1, seed, k=24):
    """members, accounts just above members, below all, above all and random ones"""
    _, _, _, acc, credited = host.entries()
    inside = np.asarray(acc)[m0:m1][np.asarray(credited)[m0:m1]]
    rng = np.random.default_rng(seed)
    q = [np.zeros((1, 4), np.uint64), np.full((1, 4), P - 1, np.uint64), rand_keys(seed, 4)]
    if len(inside):
        members = inside[rng.integers(0, len(inside), k)]
        above = members.copy()
        above[:, 3] = np.where(above[:, 3] < P - 1, above[:, 3] + np.uint64(1), above[:, 3])
        q += [members, above]
    return np.concatenate(q)


def same_everywhere(ctx, dev, host, m0=0, m1=None, seed=5, queries=None):
    """commitment, the log form on both paths and a batch of claims: device == host; returns the claims"""
    import qp_wormhole
    want = host.commit_claims(m0, m1)
    assert dev.commit_claims(m0, m1) == want
    if host.admitted:
        log_host = qp_wormhole.ledger_log_claims_root(None, host.entries(), m0, m1)
        assert qp_wormhole.ledger_log_claims_root(ctx, dev.entries(), m0, m1) == log_host
        assert log_host[:3] == (want.root, want.count, want.total)
    q = sample_queries(host, want.m0, want.m1, seed) if queries is None else queries
    d, h = dev.claims(q, m0, m1), host.claims(q, m0, m1)
    assert len(d) == len(h) == len(q)
    for a, b in zip(d, h):
        assert a == b
    assert all(qp_wormhole.check_claim(p, want.root, want.count) for p in d[:8])
    return want, d


SIZES = ["0", "1", "2", "T-1", "T", "T+1", "2*T", "2*T+1", "3*T+5"]


@pytest.mark.parametrize("extra", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_sizes(ctx, T, size, extra):
    """tile boundaries, an even and an odd run count (the unpaired run), with as many entries as rows
    and with more entries than rows"""
    A = eval(size, {"T": T})
    pis = stream_for(rand_keys(3 * A + extra, A), extra, seed=A + 7 * extra)
    if A == 0 and extra:  # a range whose entries are all double spends
        first = stream_for(rand_keys(1, 5), False, seed=1)
        pis = np.concatenate([first, first[:4]])
    dev, host = pair(ctx, pis)
    try:
        m0 = 5 if A == 0 and extra else 0
        want, _ = same_everywhere(ctx, dev, host, m0)
        assert want.count == A and (not extra or host.admitted - m0 > A)
        assert want.total == host.recount()[2] or m0
    finally:
        dev.free()
        host.free()


@pytest.mark.parametrize("name", PATTERNS)
def test_key_patterns(ctx, T, name):
    A = 2 * T + 1
    dev, host = pair(ctx, stream_for(pattern_accounts(name, A), True, seed=len(name)))
    try:
        assert same_everywhere(ctx, dev, host)[0].count == A
    finally:
        dev.free()
        host.free()


def test_carries(ctx, T):
    """2T + 1 rows; every fourth account's entries have every amount limb 0xFFFFFFFF and it is credited
    three times, so a carry crosses each limb boundary up into limb 0 of the five; every fourth has
    all-zero amounts"""
    A = 2 * T + 1
    acc = rand_keys(41, A)
    full, zero = np.arange(0, A, 4), np.arange(1, A, 4)
    limbs = np.random.default_rng(42).integers(0, 1 << 32, size=(A, 4), dtype=np.uint64)
    limbs[full] = amount_limbs(MAX_AMOUNT)
    limbs[zero] = 0
    once = transfers(rand_keys(43, A), acc, limbs)
    twice = [transfers(rand_keys(44 + i, len(full)), acc[full], limbs[full]) for i in range(2)]
    dev, host = pair(ctx, np.concatenate([once[:T], twice[0], once[T:], twice[1]]))
    try:
        q = np.concatenate([acc[full[:16]], acc[zero[:16]], acc[2:40:4]])
        want, claims = same_everywhere(ctx, dev, host, queries=q)
        assert want.count == A and want.total == host.recount()[2]
        assert all(p.found and p.total == 3 * MAX_AMOUNT for p in claims[:16])
        assert all(p.found and p.total == 0 for p in claims[16:32])
    finally:
        dev.free()
        host.free()


def test_rows_all_owned_by_entries_in_the_last_tile(ctx, T):
    """m0 > 0, and a range of 3T + 7 entries of which only the last T - 3 are credited"""
    early = stream_for(rand_keys(51, T), False, seed=51)
    doubles = transfers(early[np.random.default_rng(52).integers(0, T, 2 * T + 10), 0:4], rand_keys(53, 2 * T + 10))
    late = stream_for(rand_keys(54, T - 3), False, seed=54)
    dev, host = pair(ctx, early, np.concatenate([doubles, late]))
    try:
        want, _ = same_everywhere(ctx, dev, host, T)
        assert want.count == T - 3 and host.admitted - T == 3 * T + 7
    finally:
        dev.free()
        host.free()


def test_range_with_accounts_credited_before_and_inside(ctx, T):
    acc = rand_keys(61, T + 40)
    before = transfers(rand_keys(62, T), acc[:T])
    inside = transfers(rand_keys(63, T + 20), acc[20:])
    dev, host = pair(ctx, before, inside)
    try:
        want, claims = same_everywhere(ctx, dev, host, T, queries=acc[:60])
        assert want.count == T + 20 and [p.found for p in claims[:40]] == [False] * 20 + [True] * 20
        assert all(p.hi.first_seq >= T for p in claims[20:40])
        same_everywhere(ctx, dev, host, T - 5, 2 * T + 3)
    finally:
        dev.free()
        host.free()


@pytest.fixture(scope="module")
def pair_2T1(ctx, T):
    acc = rand_keys(71, 2 * T + 1)
    dev, host = pair(ctx, stream_for(acc, True, seed=71))
    yield dev, host, acc
    dev.free()
    host.free()


@pytest.mark.parametrize("k", [1, 8192, 8193])
def test_queries(ctx, pair_2T1, k):
    """one query, one batch of the search and one more than a batch; found, absent, below all and above all mixed"""
    dev, host, acc = pair_2T1
    rng = np.random.default_rng(k)
    q = rand_keys(100 + k, k)
    hit = rng.random(k) < 0.5
    q[hit] = acc[rng.integers(0, len(acc), int(hit.sum()))]
    q[0] = 0
    if k > 1:
        q[1] = P - 1
    _, claims = same_everywhere(ctx, dev, host, queries=q)
    assert (claims[0].pos, claims[0].lo) == (0, None)
    if k > 1:
        assert any(p.found for p in claims) and any(not p.found and p.lo and p.hi for p in claims)


def test_fresh_restored_reserved_and_recommitted(ctx, T):
    import qp_wormhole
    acc = rand_keys(81, T + 12)
    first = stream_for(acc[:T + 1], True, seed=81)
    dev, host = pair(ctx, first)
    try:
        for h in (dev, host):
            h.reserve(4 * T + len(first))
        n = host.admitted
        other = (dev.payouts(), dev.payouts_between(3, n - 2), dev.commit_log(), dev.commit_nullifiers())
        want, _ = same_everywhere(ctx, dev, host)
        times = qp_wormhole.claims_times()
        assert times is not None and len(times["merge_pass_ms"]) == 1 and all(v >= 0 for v in times["merge_pass_ms"])
        assert dev.commit_claims() == want and qp_wormhole.claims_times() == times  # the same range: nothing built
        assert (dev.payouts(), dev.payouts_between(3, n - 2), dev.commit_log(), dev.commit_nullifiers()) == other
        # restored from the published log
        r = qp_wormhole.WormholeLedger.restore(ctx, [ROOT_A], dev.entries())
        try:
            same_everywhere(ctx, r, host)
        finally:
            r.free()
        times = qp_wormhole.claims_times()  # the restored ledger's build was this thread's last
        # reserved between the commit and the claims: the commitment is its own and stands
        dev.reserve(8 * T + len(first))
        assert qp_wormhole.claims_times() == times
        q = np.concatenate([acc[:6], acc[T + 1:T + 6]])
        assert dev.claims(q) == host.claims(q)
        assert qp_wormhole.claims_times() == times
        # one more admitting cast: the closed range stands, the open range moves one tile boundary on
        more = transfers(rand_keys(182, 13),np.concatenate([acc[T + 1:], acc[:2]]))
        for h in (dev, host):
            h.cast_public(more, raw=True)
        assert dev.commit_claims(0, n) == want
        want2, _ = same_everywhere(ctx, dev, host, seed=9)
        assert want2.count == T + 12 and want2.root != want.root
        same_everywhere(ctx, dev, host, n)  # the round of the last cast alone
        assert dev.commit_log() == host.commit_log() and dev.commit_nullifiers() == host.commit_nullifiers()
    finally:
        dev.free()
        host.free()


def test_empty_ledger_and_refusals(ctx):
    import qp_wormhole
    dev = new_ledger(ctx, 8)
    try:
        assert tuple(dev.commit_claims()) == ([0, 0, 0, 0], 0, 0, 0, 0)
        p = dev.claim_for([1, 2, 3, 4])
        assert (p.found, p.pos, p.lo, p.hi) == (False, 0, None, None) and qp_wormhole.check_claim(p)
        with pytest.raises(qp_wormhole.QpError, match=r"qp_ledger_commit_claims: entries \[0, 1\) are not a range"):
            dev.commit_claims(0, 1)
        with pytest.raises(qp_wormhole.QpError, match="account at position 0 felt 3 is not a canonical"):
            dev.claims(np.array([[1, 2, 3, P]], np.uint64))
        assert dev.admitted == 0 and dev.commit_nullifiers() == ([0, 0, 0, 0], 0)
    finally:
        dev.free()
