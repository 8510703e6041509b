"""BallotBox on the device (csrc/ballot.hip: k_ballot_insert, k_ballot_resolve,
k_ballot_rebuild, k_ballot_recount): every stream of ballot_model.py under
every batching against the model and, result for result, against the host path
fed the same stream; then real voting proofs end to end: registry, prover,
verifier, box."""
import numpy as np
import pytest

from ballot_model import (BATCHINGS, COUNTED, DOUBLE_VOTE, PROOF_REJECTED, STREAMS, UNKNOWN_ROOT, WRONG_PROPOSAL,
                          run_stream)
from registry_oracle import make_keys

pytestmark = pytest.mark.gpu

PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4
OTHER = [0x2A2A2A2A2A2A2A2A] * 3 + [7]


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def host_box(proposal, roots, capacity):
    from qp_wormhole import BallotBox
    return BallotBox(None, proposal, roots, capacity=capacity)


@pytest.fixture(scope="module")
def host_results():
    """the host path's results per stream, computed once (they do not depend on the batching)"""
    return {name: run_stream(host_box, name, None) for name in STREAMS}


@pytest.mark.parametrize("batching", BATCHINGS)
@pytest.mark.parametrize("name", STREAMS)
def test_stream_matches_model_and_host_path(ctx, host_results, name, batching):
    from qp_wormhole import BallotBox
    # run_stream holds results, tally, state, entries and recount (== tally) to the model
    got = run_stream(lambda proposal, roots, cap: BallotBox(ctx, proposal, roots, capacity=cap), name, batching)
    assert got == host_results[name]


def test_voting_proofs_end_to_end(ctx):
    import qp_wormhole
    from qp_wormhole import BallotBox, QpError, VoterRegistry, WormholeVerifier
    from qp_wormhole.prover import _verifier_only
    keys = make_keys(6, 6)
    com = [VoterRegistry.commitment(k) for k in keys]
    circ = qp_wormhole.Circuit.voting()
    prover = qp_wormhole.Prover(ctx, circ, 9)
    reg = VoterRegistry.from_commitments(ctx, com[:5])
    ver = box = box_new = box_both = wver = None
    try:
        root0 = list(reg.root)
        votes = [True, False, True, True, False]
        inputs = [reg.inputs_for(keys[i], i, PROPOSAL, votes[i]) for i in range(5)]
        inputs.append(reg.inputs_for(keys[2], 2, PROPOSAL, not votes[2]))   # voter 2 again, the other vote
        inputs.append(reg.inputs_for(keys[0], 0, OTHER, True))              # another proposal
        inputs.append(reg.inputs_for(keys[4], 4, PROPOSAL, True))           # kept for the next epoch
        proofs = prover.prove_inputs(inputs)
        flipped = bytearray(proofs[1])
        flipped[100] ^= 1
        ver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=16)
        box = BallotBox(ctx, PROPOSAL, [root0], verifier=ver)
        batch = proofs[:6] + [bytes(flipped), proofs[6]]
        verdicts = ver.verify_batch(batch)
        res = [tuple(r) for r in box.cast(batch)]
        assert res[:5] == [(COUNTED, 0, i, i) for i in range(5)]
        assert res[5] == (DOUBLE_VOTE, 0, 5, 2)
        assert verdicts[6] != 0 and res[6] == (PROOF_REJECTED, verdicts[6], 6, 6)
        assert res[7] == (WRONG_PROPOSAL, 0, 7, 7)
        assert box.tally == (3, 2) and (box.cast_count, box.admitted) == (8, 6)
        assert box.recount() == (3, 2, 5, 6)
        nul = box.entries()[0]
        assert [int(x) for x in nul[2]] == inputs[2].public_inputs.nullifier
        # the same ballots through the host path
        hbox = BallotBox(None, PROPOSAL, [root0], verifier=ver)
        try:
            assert [tuple(r) for r in hbox.cast(batch)] == res and hbox.tally == box.tally
        finally:
            hbox.free()
        # a new epoch: a proof under the old root meets boxes that know only the new root, or both
        reg.append(com[5:])
        assert list(reg.root) != root0
        old = proofs[7]
        box_new = BallotBox(ctx, PROPOSAL, [reg.root], verifier=ver)
        assert [tuple(r) for r in box_new.cast([old])] == [(UNKNOWN_ROOT, 0, 0, 0)]
        box_both = BallotBox(ctx, PROPOSAL, [reg.root], verifier=ver)
        box_both.accept_root(root0)
        assert [tuple(r) for r in box_both.cast([old])] == [(COUNTED, 0, 0, 0)] and box_both.tally == (1, 0)
        # a verifier of the Wormhole circuit
        wcirc = qp_wormhole.Circuit.wormhole()
        wver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), wcirc.common_data()), max_batch=1)
        box.verifier = wver
        with pytest.raises(QpError, match="QP_ERR_ARG.*public inputs"):
            box.cast([proofs[0]])
        assert box.cast_count == 8
    finally:
        for x in (box, box_new, box_both):
            if x is not None:
                x.free()
        for x in (ver, wver):
            if x is not None:
                x.close()
        reg.free()
        prover.free()
        circ.free()
