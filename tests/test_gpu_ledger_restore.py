"""Reopening a transfer ledger from its published log and payout rounds on the
device (csrc/ledger.hip: the audit's screen, the whole-log insert and the
audit's resolve over the new ledger's tables; k_ledger_round_credit and the
payees' compaction over a round's scratch table): the cases of
test_ledger_restore.py against the same model and, result for result, against
the host path; the two paths restoring each other's logs; then real Wormhole
proofs end to end."""
import numpy as np
import pytest

from ledger_model import STREAMS
from ledger_restore_model import (EDGE_SIZES, check_block_edges, check_restore_refusals, check_restore_stream,
                                  check_round_big, check_round_identities, check_round_ranges, check_round_sizing)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_ledger(ctx):
    from qp_wormhole import WormholeLedger
    return lambda roots, padding, cap: WormholeLedger(ctx, roots, padding=padding, capacity=cap)


def host_ledger(roots, padding, capacity):
    from qp_wormhole import WormholeLedger
    return WormholeLedger(None, roots, padding=padding, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_restore_at_the_cuts(ctx, device_ledger, name):
    assert check_restore_stream(ctx, device_ledger, name) == check_restore_stream(None, host_ledger, name)


@pytest.mark.parametrize("name", ["grow", "screened", "collide_nullifiers", "collide_accounts"])
def test_restore_across_paths(ctx, device_ledger, name):
    """a device log restored on the host, and a host log restored on the device"""
    want = check_restore_stream(None, host_ledger, name)
    assert check_restore_stream(None, host_ledger, name, entries_factory=device_ledger) == want
    assert check_restore_stream(ctx, device_ledger, name, entries_factory=host_ledger) == want


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_restore_block_edges(ctx, device_ledger, n):
    assert check_block_edges(ctx, device_ledger, n) == check_block_edges(None, host_ledger, n)


def test_restore_refusals(ctx, device_ledger):
    check_restore_refusals(ctx, device_ledger)


@pytest.mark.parametrize("name", STREAMS)
def test_round_identities(ctx, device_ledger, name):
    assert check_round_identities(ctx, device_ledger, name) == check_round_identities(None, host_ledger, name)


def test_round_ranges(ctx, device_ledger):
    assert check_round_ranges(ctx, device_ledger) == check_round_ranges(None, host_ledger)


def test_round_totals_beyond_2_128(ctx, device_ledger):
    assert check_round_big(ctx, device_ledger) == check_round_big(None, host_ledger)


def test_round_sizing_and_cap(ctx, device_ledger):
    assert check_round_sizing(ctx, device_ledger) == check_round_sizing(None, host_ledger)


def test_log_only_rounds_across_paths(ctx, device_ledger):
    """the log-only form on a host ledger's entries through the device, and the reverse, equals the
    ledger form"""
    from ledger_log_model import sized_items
    from ledger_model import ROOT_A, cast_batch
    from qp_wormhole import ledger_log_payouts
    items = sized_items(600, seed=9, accounts=11)
    got = []
    for factory, other in ((device_ledger, None), (host_ledger, ctx)):
        led = factory([ROOT_A], None, 600)
        try:
            cast_batch(led, items)
            entries = led.entries()
            got.append([led.payouts_between(m0, m1) for m0, m1 in ((0, 600), (255, 513), (599, 600))])
            assert [ledger_log_payouts(other, entries, m0, m1) for m0, m1 in ((0, 600), (255, 513), (599, 600))] == got[-1]
        finally:
            led.free()
    assert got[0] == got[1]


def test_wormhole_proofs_to_restore_and_rounds(ctx):
    """real proofs through cast, the commitment, the published log audited by a fresh context and
    restored with that root; a repeat of one proof is a double spend naming the original; the two rounds
    add up to the payouts"""
    import qp_wormhole
    from qp_wormhole import WormholeLedger, WormholeVerifier, audit_ledger_log, ledger_log_payouts
    from qp_wormhole.synthetic import synthetic_inputs
    config = "standard_recursion_zk_config"
    proofs = [qp_wormhole.WormholeProver(config).commit(synthetic_inputs(60 + k, k % 3)).prove() for k in range(3)]
    pis = [[int(x) for x in p.public_inputs] for p in proofs]
    roots = [pi[4:8] for pi in pis]
    ver = WormholeVerifier(config)
    led = again = fresh = None
    try:
        led = WormholeLedger(ctx, roots, verifier=ver)
        assert [r.status for r in led.cast([p.to_bytes() for p in proofs[:2]])] == [0, 0]
        first = led.commit_log()
        assert [r.status for r in led.cast([proofs[2].to_bytes()])] == [0]
        root, n = led.commit_log()
        entries, payouts = led.entries(), led.payouts()
        rounds = [led.payouts_between(0, first[1]), led.payouts_between(first[1], n)]
        fresh = qp_wormhole.Context(0)
        assert audit_ledger_log(fresh, entries, root=root, payouts=payouts, commitments=[first]).status == 0
        assert [ledger_log_payouts(fresh, entries, 0, first[1]), ledger_log_payouts(fresh, entries, first[1], n)] == rounds
        total = {}
        for acc, t, _ in rounds[0] + rounds[1]:
            total[acc] = total.get(acc, 0) + t
        assert total == {acc: t for acc, t, _ in payouts}
        again = WormholeLedger.restore(fresh, roots, entries, verifier=ver, root=root)
        assert (again.cast_count, again.admitted, again.credited, again.accounts) == (3, 3, 3, len(payouts))
        assert again.payouts() == payouts and again.commit_log() == (root, n)
        res = again.cast([proofs[1].to_bytes()])
        assert [(r.status, r.number, r.first) for r in res] == [(6, 3, 1)]
        assert again.find(np.array([pis[1][0:4]], np.uint64)) == [1]
    finally:
        for x in (again, led):
            if x is not None:
                x.free()
        if fresh is not None:
            fresh.close()
        ver.close()
