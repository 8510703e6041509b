"""BallotBox on the host path (ctx None; csrc/ballot_table.h through
qp_ballot_box_*): every stream of ballot_model.py under every batching against
the model, the refusals (each leaving the box as it was), and one end-to-end
case with real voting proofs from the oracle prover."""
import numpy as np
import pytest

from ballot_model import (BAD_VOTE, BATCHINGS, COUNTED, DOUBLE_VOTE, PROOF_REJECTED, PROPOSAL, ROOT_A, ROOT_B, STREAMS,
                          WRONG_PROPOSAL, P, ballot, run_stream)


def host_box(proposal, roots, capacity):
    from qp_wormhole import BallotBox
    return BallotBox(None, proposal, roots, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_stream_matches_model_under_every_batching(name):
    runs = [run_stream(host_box, name, b) for b in BATCHINGS]
    for r in runs[1:]:
        assert r == runs[0]


def test_stream_branches_are_reached():
    """the crafted streams do what their names say (so the model's agreement means something)"""
    one = run_stream(host_box, "one_nullifier", None)
    assert one[0][0] == COUNTED and all(r[0] == DOUBLE_VOTE and r[3] == 0 for r in one[1:]) and len(one) == 64
    twice = run_stream(host_box, "across_batches", 64)
    assert [r[0] for r in twice] == [COUNTED] * 32 + [DOUBLE_VOTE] * 32
    assert [r[3] for r in twice[32:]] == list(range(32))
    assert all(r[0] == COUNTED for r in run_stream(host_box, "felt3_only", None))
    wrap = run_stream(host_box, "chain_wrap", 7)
    assert [r[3] for r in wrap[20:]] == list(range(20))
    many = run_stream(host_box, "many_blocks", None)
    assert sum(r[0] == COUNTED for r in many) == 2048 and sum(r[0] == DOUBLE_VOTE for r in many) == 6144
    scr = run_stream(host_box, "screened", None)
    assert [r[0] for r in scr] == [0, 3, 0, 4, 5, 2, 1, 0, 3, 4, 1, 2, 6, 2, 0, 6]
    assert scr[6][1] == 9 and scr[10][1] == 3 and [r[2] for r in scr] == list(range(16))


def snapshot(box):
    nul, num, counted, votes = box.entries()
    return (box.cast_count, box.admitted, box.capacity, box.tally, nul.tobytes(), num.tobytes(), counted.tobytes(),
            votes.tobytes(), box.recount())


def test_refusals_leave_the_box_as_it_was():
    from qp_wormhole import BallotBox, QpError
    box = host_box(PROPOSAL, [ROOT_A], 4)
    try:
        box.cast_public([ballot([1, 2, 3, i], i & 1) for i in range(3)] + [ballot([1, 2, 3, 0], 1)], reserve=False)
        before = snapshot(box)
        assert before[:4] == (4, 4, 4, (1, 2))
        # one more admitted ballot than the capacity holds, behind a rejected one: refused whole
        with pytest.raises(QpError, match="QP_ERR_ARG.*reserve"):
            box.cast_public([ballot([9, 9, 9, 9], 2), ballot([5, 5, 5, 5])], reserve=False)
        assert snapshot(box) == before
        # ballots that are not admitted need no room
        r = box.cast_public([ballot([9, 9, 9, 9], 2)], reserve=False)
        assert tuple(r[0]) == (BAD_VOTE, 0, 4, 4)
        with pytest.raises(QpError, match="QP_ERR_ARG"):
            box.reserve(3)  # below the admitted count
        with pytest.raises(QpError, match="QP_ERR_ARG"):
            box.reserve((1 << 31) + 1)
        with pytest.raises(ValueError):
            box.accept_root([1, 2, 3, P])
        with pytest.raises(ValueError, match="verdicts"):
            box.cast_public([ballot([5, 5, 5, 5])], verdicts=[0, 0])
        assert snapshot(box) == before[:0] + (5,) + before[1:]
        # with auto-reserve the same batch goes through
        r = box.cast_public([ballot([5, 5, 5, 5])])
        assert tuple(r[0]) == (COUNTED, 0, 5, 5) and box.capacity == 8 and box.tally == (2, 2)
    finally:
        box.free()
    for bad in ([1, 2, 3], [1, 2, 3, P], [1, 2, 3, -1]):
        with pytest.raises(ValueError, match="proposal_id"):
            BallotBox(None, bad, [ROOT_A])
    with pytest.raises(ValueError, match="0 accepted roots"):
        BallotBox(None, PROPOSAL, [])
    with pytest.raises(ValueError, match="65 accepted roots"):
        BallotBox(None, PROPOSAL, [[i, 0, 0, 0] for i in range(65)])
    with pytest.raises(ValueError, match="a root"):
        BallotBox(None, PROPOSAL, [[1, 2, 3, P]])
    for cap in (0, (1 << 31) + 1):
        with pytest.raises(ValueError, match="capacity"):
            BallotBox(None, PROPOSAL, [ROOT_A], capacity=cap)


def test_accept_root_twice_and_the_64_root_limit():
    from qp_wormhole import QpError
    box = host_box(PROPOSAL, [ROOT_A], 8)
    try:
        b = ballot([7, 7, 7, 7], 1, root=ROOT_B)
        assert box.cast_public([b])[0].status == 4  # unknown root
        box.accept_root(ROOT_B)
        box.accept_root(ROOT_B)
        assert tuple(box.cast_public([b])[0]) == (COUNTED, 0, 1, 1)
        for i in range(62):
            box.accept_root([i, 0, 0, 1])
        box.accept_root(ROOT_A)  # held already: no 65th
        with pytest.raises(QpError, match="QP_ERR_ARG"):
            box.accept_root([99, 0, 0, 1])
        assert box.tally == (1, 0) and box.cast_count == 2
    finally:
        box.free()


def test_default_capacity_and_growth():
    box = host_box(PROPOSAL, [ROOT_A], None)
    try:
        assert box.capacity == 1024
        pis = np.array([ballot([i, 1, 2, 3], i % 3 == 0) for i in range(1500)], dtype=np.uint64)
        res = box.cast_public(pis, raw=True)
        assert (res["status"] == 0).all() and (res["first"] == np.arange(1500)).all()
        assert box.capacity == 2048 and box.tally == (500, 1000) and box.recount() == (500, 1000, 1500, 1500)
        box.cast_public(pis[:600])
        assert box.capacity == 4096 and box.admitted == 2100 and box.tally == (500, 1000)
    finally:
        box.free()


def test_end_to_end_with_oracle_proofs():
    """real voting proofs (oracle prover, test side) through the host verifier into a host box"""
    from qp_wormhole import BallotBox, Circuit, QpError, WormholeVerifier
    from qp_wormhole.synthetic import synthetic_vote_inputs, vote_test_inputs
    from test_voting import oracle_prove
    circ = Circuit.voting()
    d = vote_test_inputs()
    proofs = []
    for data in (d, synthetic_vote_inputs(3, 3)):
        w = circ.commit(data)
        pf, vd = oracle_prove(circ, w.wires(), w.public_inputs())
        proofs.append(pf)
    cb = circ.common_data()
    good, other = proofs
    flipped = bytearray(good)
    flipped[100] ^= 1
    ver = WormholeVerifier(circuit_data=(vd[:-len(cb)], cb), device=None, max_batch=4)
    box = BallotBox(None, d.public_inputs.proposal_id, [d.public_inputs.merkle_root], verifier=ver)
    try:
        want = ver.verify_batch([good, good, bytes(flipped), other])
        assert want[0] == want[1] == want[3] == 0 and want[2] != 0
        res = box.cast([good, good, bytes(flipped), other])
        assert [tuple(r) for r in res] == [(COUNTED, 0, 0, 0), (DOUBLE_VOTE, 0, 1, 0), (PROOF_REJECTED, want[2], 2, 2),
                                           (WRONG_PROPOSAL, 0, 3, 3)]
        assert box.tally == (1, 0) and (box.cast_count, box.admitted) == (4, 2)
        nul, num, counted, votes = box.entries()
        assert [int(x) for x in nul[0]] == d.public_inputs.nullifier and list(counted) == [True, False]
        assert box.cast([]) == []
        # a verifier of another circuit is an argument error
        wcirc = Circuit.wormhole()
        wver = WormholeVerifier(circuit_data=(vd[:-len(cb)], wcirc.common_data()), device=None, max_batch=1)
        try:
            box.verifier = wver
            with pytest.raises(QpError, match="QP_ERR_ARG.*public inputs"):
                box.cast([good])
        finally:
            wver.close()
        assert box.cast_count == 4
    finally:
        box.free()
        ver.close()
