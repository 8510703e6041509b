"""WormholeLedger on the device (csrc/ledger.hip: screen, scan, pack, insert,
resolve and credit, rebuild, find, totals, the payouts' compaction, recount):
every stream of ledger_model.py under every batching against the model and,
result for result, against the host path fed the same stream; one-batch streams
whose admitted transfers cross block boundaries; the most contended account;
then real Wormhole proofs end to end, per proof and through an aggregated root."""
import numpy as np
import pytest

from ledger_model import (BATCHINGS, CREDITED, DOUBLE_SPEND, MAX_AMOUNT, PADDING, PROOF_REJECTED, ROOT_A, RUN_STREAMS,
                          STREAMS, account_bytes, run_stream, transfer)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def host_ledger(roots, padding, capacity):
    from qp_wormhole import WormholeLedger
    return WormholeLedger(None, roots, padding=padding, capacity=capacity)


@pytest.fixture(scope="module")
def host_results():
    """the host path's results per stream, computed once (they do not depend on the batching)"""
    return {name: run_stream(host_ledger, name, None) for name in STREAMS + RUN_STREAMS}


def device_factory(ctx):
    from qp_wormhole import WormholeLedger
    return lambda roots, padding, cap: WormholeLedger(ctx, roots, padding=padding, capacity=cap)


@pytest.mark.parametrize("batching", BATCHINGS)
@pytest.mark.parametrize("name", STREAMS)
def test_stream_matches_model_and_host_path(ctx, host_results, name, batching):
    # run_stream holds results, state, entries, find, payouts, totals and recount to the model, and
    # find, payouts and totals to themselves across every reserve
    assert run_stream(device_factory(ctx), name, batching) == host_results[name]


@pytest.mark.parametrize("name", RUN_STREAMS)
def test_stable_pack_across_block_boundaries(ctx, host_results, name):
    """255, 256, 257 and 513 transfers in one batch, admitted and rejected ones alternating in runs
    of 1, 3 and 64, and 513 of which only the last is admitted: the log's order is the stream's"""
    got = run_stream(device_factory(ctx), name, None)
    assert got == host_results[name]
    if name == "runs_513_last":
        assert [r[0] in (CREDITED, DOUBLE_SPEND) for r in got] == [False] * 512 + [True]


def test_one_account_credited_by_4096_transfers_in_one_batch(ctx):
    """the most contended atomics: every limb 0xFFFFFFFF, 16,384 adds onto one slot's four sums"""
    from qp_wormhole import WormholeLedger
    led = WormholeLedger(ctx, [ROOT_A], capacity=4096)
    try:
        acc = [7, 8, 9, 10]
        pis = np.array([transfer([i, 1, 2, 3], MAX_AMOUNT, acc) for i in range(4096)], dtype=np.uint64)
        res = led.cast_public(pis, reserve=False, raw=True)
        assert (res["status"] == CREDITED).all() and (res["first"] == np.arange(4096)).all()
        assert led.payouts() == [(account_bytes(acc), 4096 * MAX_AMOUNT, 0)]
        assert led.total_for(acc) == 4096 * MAX_AMOUNT and led.recount() == (4096, 4096, 4096 * MAX_AMOUNT)
        assert (led.credited, led.accounts) == (4096, 1)
    finally:
        led.free()


def test_wormhole_proofs_end_to_end(ctx):
    import qp_wormhole
    from qp_wormhole import WormholeLedger, WormholeVerifier
    from qp_wormhole.synthetic import synthetic_inputs
    config = "standard_recursion_zk_config"
    leaves = [qp_wormhole.WormholeProver(config).commit(synthetic_inputs(40 + k, k % 3)).prove() for k in range(5)]
    pis = [[int(x) for x in p.public_inputs] for p in leaves]
    roots = [pi[4:8] for pi in pis]
    ver = WormholeVerifier(config)
    led = hled = aled = None
    try:
        flipped = bytearray(leaves[1].to_bytes())
        flipped[100] ^= 1
        batch = [p.to_bytes() for p in leaves] + [leaves[2].to_bytes(), bytes(flipped)]
        verdicts = ver.verify_batch(batch)
        assert verdicts[:6] == [0] * 6 and verdicts[6] != 0
        led = WormholeLedger(ctx, roots, verifier=ver)
        res = [tuple(r) for r in led.cast(batch)]
        assert res == [(CREDITED, 0, i, i) for i in range(5)] + [(DOUBLE_SPEND, 0, 5, 2),
                                                                  (PROOF_REJECTED, verdicts[6], 6, 6)]
        assert (led.cast_count, led.admitted, led.credited) == (7, 6, 5)
        want = {}
        for pi in pis:
            a = account_bytes(pi[12:16])
            want[a] = want.get(a, 0) + sum(x << (96 - 32 * i) for i, x in enumerate(pi[8:12]))
        pay = led.payouts()
        assert {a: t for a, t, _ in pay} == want and len(pay) == len(want)
        assert led.find([pi[0:4] for pi in pis]) == list(range(5))
        assert led.recount() == (5, 6, sum(want.values()))
        # the same proofs through the host path
        hled = WormholeLedger(None, roots, verifier=ver)
        assert [tuple(r) for r in hled.cast(batch)] == res and hled.payouts() == pay
        # an aggregated root of the five and three padding proofs into a fresh ledger that knows the padding
        agg = qp_wormhole.WormholeProofAggregator.default()
        for p in leaves:
            agg.push_proof(p)
        root = agg.aggregate()
        aled = WormholeLedger(ctx, roots, padding=WormholeLedger.padding_of(agg))
        res = aled.cast_aggregated(agg, root)
        assert [tuple(r) for r in res] == [(CREDITED, 0, i, i) for i in range(5)] + [(PADDING, 0, i, i) for i in (5, 6, 7)]
        assert aled.payouts() == pay
        # the same root again
        again = aled.cast_aggregated(agg, root)
        assert [tuple(r) for r in again] == [(DOUBLE_SPEND, 0, 8 + i, i) for i in range(5)] + \
            [(PADDING, 0, 8 + i, 8 + i) for i in (5, 6, 7)]
        assert aled.payouts() == pay and (aled.cast_count, aled.admitted, aled.credited) == (16, 10, 5)
    finally:
        for x in (led, hled, aled):
            if x is not None:
                x.free()
        ver.close()
