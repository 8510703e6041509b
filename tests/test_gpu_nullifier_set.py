"""The nullifier-set commitment on the device (csrc/nullifier_set.hip: select,
tile sort, merge passes, duplicates, leaves, search, gather; the levels and
paths through the accumulator tree's launchers): the device equals the host
path of the same library word for word (order, root, found, pos, both slots),
at the shapes where a sort or a merge breaks, T = qp_nullifier_set_tile().  The
host path is held to the plain-Python model by test_nullifier_set.py."""
import random

import numpy as np
import pytest

from nullifier_set_model import (PATTERNS, P, as_tuple, cast_keys, make_handle, pattern_keys, random_keys)

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
    rng = np.random.default_rng(seed)
    return rng.integers(0, P, size=(n, 4), dtype=np.uint64)


def both_roots(ctx, nul, member):
    import qp_wormhole
    host = qp_wormhole.nullifier_set_root(None, (nul, member))
    dev = qp_wormhole.nullifier_set_root(ctx, (nul, member))
    assert dev == host
    return host


SIZES = ["0", "1", "2", "T-1", "T", "T+1", "2*T", "2*T+1", "3*T+5", "5*T+3"]


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_sizes(ctx, T, size, interleaved):
    """tile boundaries, an even and an odd run count (the unpaired run), with n = m and with
    non-members between the members"""
    m = eval(size, {"T": T})
    n = 2 * m + 3 if interleaved else m
    nul = rand_keys(m * 2 + interleaved, n)
    member = np.ones(n, np.uint8)
    if interleaved:
        member[:] = 0
        member[np.random.default_rng(7).choice(n, m, replace=False)] = 1
    root, got_m, order, dup = both_roots(ctx, nul, member)
    assert got_m == m and dup is None
    keys = [tuple(int(x) for x in nul[s]) for s in order]
    assert keys == sorted(keys) and sorted(order) == [int(s) for s in np.flatnonzero(member)]


@pytest.mark.parametrize("name", [p for p in PATTERNS if p != "one_home"])
def test_key_patterns(ctx, T, name):
    m = 2 * T + 1
    nul = np.array(pattern_keys(name, m), dtype=np.uint64)
    root, got_m, order, dup = both_roots(ctx, nul, np.ones(m, np.uint8))
    assert got_m == m and dup is None
    keys = [tuple(int(x) for x in nul[s]) for s in order]
    assert keys == sorted(keys)


def test_members_all_in_the_last_tile(ctx, T):
    n = 3 * T + 7
    nul = rand_keys(11, n)
    member = np.zeros(n, np.uint8)
    member[n - T + 3:] = 1
    assert both_roots(ctx, nul, member)[1] == T - 3


def test_duplicates_across_a_tile_boundary(ctx, T):
    """two equal keys whose members land in different tiles of the sort; the lowest offender wins"""
    n = 2 * T + 10
    nul = rand_keys(13, n)
    nul[T + 5] = nul[3]          # tiles 1 and 0
    nul[2 * T + 1] = nul[T - 1]  # tiles 2 and 0
    member = np.ones(n, np.uint8)
    assert both_roots(ctx, nul, member)[3] == T + 5
    member[T + 5] = 0  # the first pair is gone; the member ranks past it move down by one
    assert both_roots(ctx, nul, member)[3] == 2 * T + 1
    nul[7] = nul[8]  # equal neighbours inside one tile
    assert both_roots(ctx, nul, member)[3] == 8


def proofs_equal(dev, host, keys):
    d, h = dev.nullifier_proofs(keys), host.nullifier_proofs(keys)
    assert len(d) == len(h) == len(keys)
    for a, b in zip(d, h):
        assert a == b
    return d


@pytest.fixture(scope="module")
def pair_2T1(ctx, T):
    """a device ledger and a host ledger with the same 2T + 1 members and some double spends"""
    m = 2 * T + 1
    keys = rand_keys(17, m)
    stream = np.concatenate([keys[:T], keys[5:40], keys[T:]])
    dev, host = make_handle("ledger", ctx, len(stream)), make_handle("ledger", None, len(stream))
    for h in (dev, host):
        cast_keys("ledger", h, stream)
    yield dev, host, keys
    dev.free()
    host.free()


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1025])
def test_queries(pair_2T1, k):
    """found, absent, below all and above all mixed, at one wave, either side of it, and several blocks"""
    dev, host, keys = pair_2T1
    rng = np.random.default_rng(k)
    q = rand_keys(100 + k, k)
    hit = rng.random(k) < 0.5
    q[hit] = keys[rng.integers(0, len(keys), int(hit.sum()))]
    q[0] = 0
    if k > 1:
        q[1] = P - 1
    assert dev.commit_nullifiers() == host.commit_nullifiers()
    ps = proofs_equal(dev, host, q)
    if k >= 63:
        assert any(p.found for p in ps) and any(not p.found and p.lo and p.hi for p in ps)
    assert dev.check_nullifier_proof(ps[0]) and dev.check_nullifier_proof(ps[-1])
    assert (ps[0].pos, ps[0].lo) == (0, None)


def test_queries_batch_boundary(pair_2T1):
    """8193 keys: one more than the search's batch"""
    dev, host, keys = pair_2T1
    q = np.concatenate([keys[:4096], rand_keys(23, 4097)])
    proofs_equal(dev, host, q)


@pytest.mark.parametrize("kind", ["box", "ledger"])
def test_handles_fresh_restored_reserved_and_recommitted(ctx, T, kind):
    import qp_wormhole
    rng = random.Random("gpu handles " + kind)
    keys = random_keys(rng, T + 12)
    first = keys[:T + 1] + keys[3:9]  # T + 1 members and six doubles
    dev, host = make_handle(kind, ctx, 2 * T), make_handle(kind, None, 2 * T)
    try:
        for h in (dev, host):
            cast_keys(kind, h, first)
        want = host.commit_nullifiers()
        assert dev.commit_nullifiers() == want and want[1] == T + 1
        assert dev.commit_nullifiers() == want  # cached
        assert dev.commit_log() == host.commit_log()
        q = keys[:5] + keys[T + 1:T + 6] + [[0, 0, 0, 0], [P - 1] * 4]
        proofs_equal(dev, host, q)
        # restored from the published log
        if kind == "box":
            r = qp_wormhole.BallotBox.restore(ctx, [0x2A2A2A2A2A2A2A2A] * 4, [[11, 12, 13, P - 1]], dev.entries())
        else:
            r = qp_wormhole.WormholeLedger.restore(ctx, [[11, 12, 13, P - 1]], dev.entries())
        try:
            assert r.commit_nullifiers() == want
            proofs_equal(r, host, q)
        finally:
            r.free()
        # after a reserve the set stands, and proofs still come from it
        dev.reserve(4 * T)
        assert dev.commit_nullifiers() == want
        proofs_equal(dev, host, q)
        # one more admitting cast: a second commit, one tile boundary further
        for h in (dev, host):
            cast_keys(kind, h, keys[T + 1:] + keys[:2])
        want2 = host.commit_nullifiers()
        assert dev.commit_nullifiers() == want2 and want2[1] == T + 12 and want2 != want
        for p in proofs_equal(dev, host, q):
            assert dev.check_nullifier_proof(p)
        assert dev.commit_log() == host.commit_log()
    finally:
        dev.free()
        host.free()


def test_one_home_slot(ctx, T):
    """every member's key has the same home slot of the handle's table: the table's chain is as long
    as the set, the sort does not care"""
    m = 2 * T + 1
    slots = 1
    while slots < 2 * m:
        slots *= 2
    keys = pattern_keys("one_home", m, slots)
    dev, host = make_handle("ledger", ctx, m), make_handle("ledger", None, m)
    try:
        for h in (dev, host):
            assert set(cast_keys("ledger", h, keys)) == {0}
        assert dev.commit_nullifiers() == host.commit_nullifiers()
        proofs_equal(dev, host, keys[:3] + [[5, 0, 0, 0]])
    finally:
        dev.free()
        host.free()


def test_empty_handle_and_stage_times(ctx, T):
    import qp_wormhole
    dev = make_handle("box", ctx, 8)
    try:
        assert dev.commit_nullifiers() == ([0, 0, 0, 0], 0)
        p = dev.nullifier_proof_for([1, 2, 3, 4])
        assert as_tuple(p) == (False, 0, None, None) and dev.check_nullifier_proof(p)
    finally:
        dev.free()
    both_roots(ctx, rand_keys(3, 4 * T), np.ones(4 * T, np.uint8))
    t = qp_wormhole.nullifier_set_times()
    assert t is not None and len(t["merge_pass_ms"]) == 2 and all(v >= 0 for v in t["merge_pass_ms"])
