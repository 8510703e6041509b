"""The ballot box's log commitment on the device (csrc/ballot.hip:
k_ballot_leaves, k_ballot_find, k_ballot_gather; the levels and paths through
the registry's launchers): the cases of test_ballot_receipts.py against the
same model and, result for result, against the host path; then real voting
proofs end to end: registry, prover, verifier, box, receipts."""
import numpy as np
import pytest

from ballot_receipt_model import (SIZES, STREAMS, check_find, check_receipt_rules, check_size, run_commit_stream)
from registry_oracle import make_keys

pytestmark = pytest.mark.gpu

PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4
OTHER = [0x2A2A2A2A2A2A2A2A] * 3 + [7]
NPI, PI_NULLIFIER = 13, 9  # a voting proof's public inputs: proposal[0:4] root[4:8] vote[8] nullifier[9:13]


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_box(ctx):
    from qp_wormhole import BallotBox
    return lambda proposal, roots, cap: BallotBox(ctx, proposal, roots, capacity=cap)


def host_box(proposal, roots, capacity):
    from qp_wormhole import BallotBox
    return BallotBox(None, proposal, roots, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_root_matches_model_and_host_path(device_box, name):
    """batchings 7 and whole commit after every batch, 64 once at the end; the
    final commitment is equal across the three and equal to the host path's, and
    so are the receipts of the first, a middle and the last entry"""
    finals = []
    for batching, every in ((7, True), (None, True), (64, False)):
        root, n, model, logm, box = run_commit_stream(device_box, name, batching, every)
        try:
            seqs = sorted({0, n // 2, n - 1})
            finals.append((root, n, [tuple(r) for r in box.receipts(seqs)]))
        finally:
            box.free()
    assert finals[0] == finals[1] == finals[2]
    root, n, model, logm, box = run_commit_stream(host_box, name, 64, False)
    try:
        assert (root, n, [tuple(r) for r in box.receipts(seqs)]) == finals[0]
    finally:
        box.free()


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_promoted_nodes(device_box, n):
    assert check_size(device_box, n) == check_size(host_box, n)


def test_find(device_box):
    assert check_find(device_box) == check_find(host_box)


def test_receipt_rules(device_box):
    assert check_receipt_rules(device_box) == check_receipt_rules(host_box)


def test_voting_proofs_to_receipts(ctx):
    import qp_wormhole
    from qp_wormhole import BallotBox, VoterRegistry, WormholeVerifier
    from qp_wormhole.prover import _verifier_only
    keys = make_keys(5, 6)
    com = [VoterRegistry.commitment(k) for k in keys]
    circ = qp_wormhole.Circuit.voting()
    prover = qp_wormhole.Prover(ctx, circ, 7)
    reg = VoterRegistry.from_commitments(ctx, com)
    ver = box = None
    try:
        votes = [True, False, True, True, False]
        inputs = [reg.inputs_for(keys[i], i, PROPOSAL, votes[i]) for i in range(5)]
        inputs.append(reg.inputs_for(keys[2], 2, PROPOSAL, not votes[2]))   # voter 2 again, the other vote
        inputs.append(reg.inputs_for(keys[0], 0, OTHER, True))              # another proposal
        proofs = prover.prove_inputs(inputs)
        ver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=16)
        box = BallotBox(ctx, PROPOSAL, [list(reg.root)], verifier=ver)
        res = box.cast(proofs)
        assert [r.status for r in res] == [0, 0, 0, 0, 0, 6, 3]
        # what the operator publishes
        root, n = box.commit_log()
        assert n == box.admitted == 6 and box.tally == (3, 2)
        # each voter reads their nullifier from their own proof: the 13 public inputs are its last 104 bytes
        nuls = [np.frombuffer(bytes(p)[-8 * NPI:], "<u8")[PI_NULLIFIER:PI_NULLIFIER + 4].tolist() for p in proofs]
        assert nuls == [[int(x) for x in inp.public_inputs.nullifier] for inp in inputs]
        for i in range(5):
            r = box.receipt_for(nuls[i])
            assert (r.seq, r.number, r.vote, r.counted) == (i, i, votes[i], True)
            assert r.nullifier == nuls[i] and (r.root, r.n) == (root, n)
            assert BallotBox.check_receipt(r, root, n)
        # the voter who voted twice gets the receipt of the first ballot; the second is in the log, not counted
        assert nuls[5] == nuls[2] and box.receipt_for(nuls[5]).seq == 2
        second = box.receipts([5])[0]
        assert (second.number, second.vote, second.counted) == (5, not votes[2], False)
        assert BallotBox.check_receipt(second, root, n)
        assert box.receipt_for(nuls[6]) is None  # the other proposal's nullifier was never admitted
    finally:
        if box is not None:
            box.free()
        if ver is not None:
            ver.close()
        reg.free()
        prover.free()
        circ.free()
