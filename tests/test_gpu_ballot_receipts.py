"""The ballot box's log commitment on the device (csrc/ballot.hip:
k_ballot_leaves, k_ballot_find, k_ballot_gather; the levels and paths through
the accumulator tree's launchers, csrc/acc_tree.hip): the cases of test_ballot_receipts.py against the
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


@pytest.mark.parametrize("hook", [None, "registry_row=0"], ids=["default", "one_lane"])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129])
def test_one_tree_serves_log_and_registry(ctx, device_box, monkeypatch, hook, n):
    """The ballot log and the voter registry are two clients of one accumulator
    tree (csrc/acc_tree.h): a commitment registry built from a committed log's
    leaves (the model's leaf function over `entries`) has the log's root, and
    its paths_raw are the receipts' buffers bit for bit.  Sizes: no parent, one
    pair, a promoted leaf, ACC_FOLD_MAX = 64 on the leaf level (64, 65) and on
    the level above (129).  Every log of at least two entries holds double
    votes (entry i = 1 mod 4 repeats entry i - 1's nullifier with the other
    vote); a log of one entry cannot.  With the one-lane form (registry_row=0)
    and the default, which governs both trees."""
    import ctypes

    from ballot_model import ROOT_A, ballot, cast_batch
    from ballot_receipt_model import leaf
    from qp_wormhole import VoterRegistry
    from qp_wormhole._native import lib
    from qp_wormhole.ballot import DOUBLE_VOTE, PATH_SLOTS
    if hook:
        monkeypatch.setenv("QPGPU_PATHS", hook)
    else:
        monkeypatch.delenv("QPGPU_PATHS", raising=False)
    rng = np.random.default_rng(1000 + n)
    nuls = rng.integers(0, 0xFFFFFFFF00000001, size=(n, 4), dtype=np.uint64).tolist()
    doubles = [i for i in range(n) if i % 4 == 1]
    for i in doubles:
        nuls[i] = nuls[i - 1]
    box = device_box(PROPOSAL, [ROOT_A], n)
    reg = None
    try:
        res = cast_batch(box, [(ballot(k, i & 1, PROPOSAL), 0) for i, k in enumerate(nuls)])
        assert [i for i, r in enumerate(res) if r.status == DOUBLE_VOTE] == doubles and (n < 2 or doubles)
        root, committed = box.commit_log()
        assert committed == n == box.admitted
        nul, num, counted, votes = box.entries()
        assert nul.tolist() == nuls and [i for i in range(n) if not counted[i]] == doubles
        leaves = [leaf((nul[i].tolist(), int(num[i]), bool(counted[i]), bool(votes[i]))) for i in range(n)]
        reg = VoterRegistry.from_commitments(ctx, leaves)
        assert [int(x) for x in reg.root] == root
        seqs = np.array(sorted({0, n // 2, n - 1}), dtype=np.uint64)
        k = len(seqs)
        sib, bits, depth = reg.paths_raw(seqs)
        rsib = np.full((k, PATH_SLOTS, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)  # every slot is written
        rbits, rdepth = np.full(k, 0xFFFFFFFF, np.uint32), np.full(k, 0xFFFFFFFF, np.uint32)
        rleaf, rroot, rn = np.zeros((k, 4), np.uint64), np.zeros(4, np.uint64), ctypes.c_uint64()
        assert lib().qp_ballot_box_receipts(box.h, seqs.ctypes.data, k, rsib.ctypes.data, rbits.ctypes.data,
                                            rdepth.ctypes.data, rleaf.ctypes.data, rroot.ctypes.data,
                                            ctypes.byref(rn)) == 0
        assert (rroot.tolist(), rn.value) == (root, n)
        assert rsib.tobytes() == sib.tobytes() and rbits.tobytes() == bits.tobytes()
        assert rdepth.tobytes() == depth.tobytes()
        assert rleaf.tolist() == [leaves[int(s)] for s in seqs]
    finally:
        if reg is not None:
            reg.free()
        box.free()


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
