"""WormholeLedger on the host path (ctx None; csrc/ledger_table.h through
qp_ledger_*): every stream of ledger_model.py under every batching against the
model, the crafted streams' branches, the refusals (each leaving the ledger as
it was), growth, and the empty cases."""
import numpy as np
import pytest

from ledger_model import (BAD_AMOUNT, BATCHINGS, CREDITED, DOUBLE_SPEND, MALFORMED, MAX_AMOUNT, PADDING, PROOF_REJECTED,
                          ROOT_A, ROOT_B, RUN_STREAMS, STREAMS, UNKNOWN_ROOT, P, account_bytes, make_stream, run_stream,
                          transfer)


def host_ledger(roots, padding, capacity):
    from qp_wormhole import WormholeLedger
    return WormholeLedger(None, roots, padding=padding, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_stream_matches_model_under_every_batching(name):
    runs = [run_stream(host_ledger, name, b) for b in BATCHINGS]
    for r in runs[1:]:
        assert r == runs[0]


@pytest.mark.parametrize("name", RUN_STREAMS)
def test_run_streams_match_model(name):
    assert run_stream(host_ledger, name, None) == run_stream(host_ledger, name, 7)


def test_stream_branches_are_reached():
    """the crafted streams do what their names say (so the model's agreement means something)"""
    one = run_stream(host_ledger, "one_nullifier", None)
    assert one[0][0] == CREDITED and all(r[0] == DOUBLE_SPEND and r[3] == 0 for r in one[1:]) and len(one) == 64
    twice = run_stream(host_ledger, "across_batches", 64)
    assert [r[0] for r in twice] == [CREDITED] * 32 + [DOUBLE_SPEND] * 32
    assert [r[3] for r in twice[32:]] == list(range(32))
    scr = run_stream(host_ledger, "screened", None)
    assert [r[0] for r in scr] == [CREDITED, PROOF_REJECTED, MALFORMED, PADDING, BAD_AMOUNT, UNKNOWN_ROOT, CREDITED,
                                   DOUBLE_SPEND, BAD_AMOUNT, PROOF_REJECTED, MALFORMED, CREDITED, DOUBLE_SPEND, MALFORMED,
                                   CREDITED, CREDITED]
    assert scr[1][1] == 4 and scr[9][1] == 9 and [r[2] for r in scr] == list(range(16))
    assert scr[7][3] == 6 and scr[12][3] == 0  # the double of the transfer whose first copy had an unknown root
    assert [r[0] for r in run_stream(host_ledger, "padding_known", None)] == [PADDING] * 4 + [CREDITED] + [PADDING] * 4
    # the trap: a ledger that does not know the padding inputs pays the dummy once
    assert [r[0] for r in run_stream(host_ledger, "padding_unknown", None)] == \
        [CREDITED] + [DOUBLE_SPEND] * 3 + [CREDITED] + [DOUBLE_SPEND] * 4
    col = run_stream(host_ledger, "collide_nullifiers", None)
    assert [r[0] for r in col] == [0, 0, 0, 6, 6, 0, 6, 6] and [r[3] for r in col] == [0, 1, 2, 1, 2, 5, 0, 5]
    assert all(r[0] == CREDITED for r in run_stream(host_ledger, "collide_accounts", 1))
    assert all(r[0] not in (CREDITED, DOUBLE_SPEND) for r in run_stream(host_ledger, "rejected_only", None))
    many = run_stream(host_ledger, "many_blocks", None)
    assert sum(r[0] == CREDITED for r in many) == 2048 and sum(r[0] == DOUBLE_SPEND for r in many) == 4096
    last = run_stream(host_ledger, "runs_513_last", None)
    assert [r[0] for r in last[-2:]] != [CREDITED] * 2 and last[-1][0] == CREDITED
    assert sum(r[0] in (CREDITED, DOUBLE_SPEND) for r in last) == 1


def test_collisions_sit_where_the_home_slot_rule_puts_them():
    """capacity 4, 8 slots: the crafted keys share home slot 7, so the chain wraps to slot 0"""
    for name, at in (("collide_nullifiers", 0), ("collide_accounts", 12)):
        cap, _, _, items = make_stream(name)
        keys = [tuple(it[0][at:at + 4]) for it in items if it[0] != "reserve"][:3]
        assert cap == 4 and len(set(keys)) == 3 and [k[0] & 7 for k in keys] == [7, 7, 7]
        assert keys[0][0] == keys[2][0] and keys[0][:3] == keys[2][:3] and keys[0][3] != keys[2][3]


def test_totals_carry_out_of_every_limb_and_beyond_128_bits():
    led = host_ledger([ROOT_A], None, 1024)
    try:
        acc = [7, 7, 7, 7]
        pis = np.array([transfer([i, 1, 2, 3], MAX_AMOUNT, acc) for i in range(513)], dtype=np.uint64)
        res = led.cast_public(pis, raw=True)
        assert (res["status"] == CREDITED).all()
        assert led.total_for(acc) == 513 * MAX_AMOUNT and led.total_for(acc) >> 128
        assert led.payouts() == [(account_bytes(acc), 513 * MAX_AMOUNT, 0)]
        led.cast_public([transfer([1000, 1, 2, 3], 0, [8, 8, 8, 8])])
        assert led.payouts()[1] == (account_bytes([8, 8, 8, 8]), 0, 513) and led.totals_for([[8, 8, 8, 8]]) == [0]
        assert led.recount() == (514, 514, 513 * MAX_AMOUNT)
    finally:
        led.free()


def snapshot(led):
    nul, num, amt, acc, credited = led.entries()
    return (led.cast_count, led.admitted, led.credited, led.accounts, led.capacity, nul.tobytes(), num.tobytes(), amt,
            acc.tobytes(), credited.tobytes(), led.payouts(), led.recount())


def test_refusals_leave_the_ledger_as_it_was():
    from qp_wormhole import QpError, WormholeLedger
    led = host_ledger([ROOT_A], None, 4)
    try:
        led.cast_public([transfer([1, 2, 3, i], 10 + i, [5, 5, 5, i & 1]) for i in range(3)] +
                        [transfer([1, 2, 3, 0], 99)], reserve=False)
        before = snapshot(led)
        assert before[:5] == (4, 4, 3, 2, 4)
        # one more admitted transfer than the capacity holds, behind a rejected one: refused whole
        with pytest.raises(QpError, match="QP_ERR_ARG.*reserve"):
            led.cast_public([transfer([9, 9, 9, 9], root=ROOT_B), transfer([5, 5, 5, 5])], reserve=False)
        assert snapshot(led) == before
        # transfers that are not admitted need no room
        r = led.cast_public([transfer([9, 9, 9, 9], root=ROOT_B)], reserve=False)
        assert tuple(r[0]) == (UNKNOWN_ROOT, 0, 4, 4)
        with pytest.raises(QpError, match="QP_ERR_ARG"):
            led.reserve(3)  # below the admitted count
        with pytest.raises(QpError, match="QP_ERR_ARG"):
            led.reserve((1 << 31) + 1)
        with pytest.raises(ValueError):
            led.accept_root([1, 2, 3, P])
        with pytest.raises(ValueError, match="verdicts"):
            led.cast_public([transfer([5, 5, 5, 5])], verdicts=[0, 0])
        with pytest.raises(QpError, match="QP_ERR_ARG.*canonical"):
            led.find([[1, 2, 3, P]])
        with pytest.raises(ValueError, match="verifier"):
            led.cast([b"x"])
        assert snapshot(led) == (5,) + before[1:]
        # with auto-reserve the same batch goes through
        r = led.cast_public([transfer([5, 5, 5, 5], 7, [5, 5, 5, 0])])
        assert tuple(r[0]) == (CREDITED, 0, 5, 5) and led.capacity == 8 and led.total_for([5, 5, 5, 0]) == 10 + 12 + 7
    finally:
        led.free()
    with pytest.raises(ValueError, match="0 accepted roots"):
        WormholeLedger(None, [])
    with pytest.raises(ValueError, match="4097 accepted roots"):
        WormholeLedger(None, [[i, 0, 0, 0] for i in range(4097)])
    with pytest.raises(ValueError, match="a root"):
        WormholeLedger(None, [[1, 2, 3, P]])
    with pytest.raises(ValueError, match="padding"):
        WormholeLedger(None, [ROOT_A], padding=[0] * 15)
    for cap in (0, (1 << 31) + 1):
        with pytest.raises(ValueError, match="capacity"):
            WormholeLedger(None, [ROOT_A], capacity=cap)


def test_accept_root_twice_many_roots_and_the_limit():
    from qp_wormhole import QpError
    led = host_ledger([ROOT_A], None, 8)
    try:
        t = transfer([7, 7, 7, 7], 3, root=ROOT_B)
        assert led.cast_public([t])[0].status == UNKNOWN_ROOT
        led.accept_root(ROOT_B)
        led.accept_root(ROOT_B)
        assert tuple(led.cast_public([t])[0]) == (CREDITED, 0, 1, 1)
        for i in range(4094):
            led.accept_root([(i * 7919) % 4099, i, 0, 1])
        led.accept_root(ROOT_A)  # held already: no 4097th
        with pytest.raises(QpError, match="QP_ERR_ARG"):
            led.accept_root([99, 0, 0, 2])
        # every one of the 4096 is found, a neighbour of one is not
        rows = [transfer([100 + i, 0, 0, 0], 1, root=[(i * 7919) % 4099, i, 0, 1]) for i in (0, 1, 2047, 4093)]
        rows.append(transfer([200, 0, 0, 0], 1, root=[(5 * 7919) % 4099, 5, 0, 2]))
        assert [r.status for r in led.cast_public(rows)] == [CREDITED] * 4 + [UNKNOWN_ROOT]
        assert led.credited == 5 and led.cast_count == 7
    finally:
        led.free()


def test_default_capacity_growth_and_empty_calls():
    led = host_ledger([ROOT_A], None, None)
    try:
        assert led.capacity == 1024
        assert led.cast_public([]) == [] and led.cast_public(np.zeros((0, 16), np.uint64)) == []
        assert led.payouts() == [] and led.recount() == (0, 0, 0) and led.find([]) == [] and led.totals_for([]) == []
        assert led.entries()[2] == [] and (led.cast_count, led.admitted, led.accounts) == (0, 0, 0)
        pis = np.array([transfer([i, 1, 2, 3], i, [i % 10, 0, 0, 0]) for i in range(1500)], dtype=np.uint64)
        res = led.cast_public(pis, raw=True)
        assert (res["status"] == 0).all() and (res["first"] == np.arange(1500)).all()
        assert led.capacity == 2048 and led.accounts == 10 and led.recount() == (1500, 1500, sum(range(1500)))
        assert [p[2] for p in led.payouts()] == list(range(10))
        assert led.total_for([3, 0, 0, 0]) == sum(range(3, 1500, 10))
        led.cast_public(pis[:600])
        assert led.capacity == 4096 and led.admitted == 2100 and led.credited == 1500
        # a batch with nothing admitted changes the cast count alone
        before = (led.admitted, led.credited, led.payouts())
        assert all(r.status == PROOF_REJECTED for r in led.cast_public(pis[:5], verdicts=[3] * 5))
        assert (led.admitted, led.credited, led.payouts()) == before and led.cast_count == 2105
    finally:
        led.free()
