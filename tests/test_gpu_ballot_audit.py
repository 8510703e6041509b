"""The audit of a published ballot log, prefix roots and restore on the device
(csrc/ballot_audit.hip: k_audit_screen, k_audit_resolve, with ballot.hip's
k_ballot_insert over the whole log and k_ballot_leaves; csrc/acc_tree.hip:
k_acc_prefix_roots): the cases of test_ballot_audit.py with a context, against
the same model and, report for report, against the host path; then real voting
proofs end to end: registry, prover, verifier, box, a published log audited by
a context that never saw the box, a restore, one more cast."""
import numpy as np
import pytest

from ballot_audit_model import (SIZES, check_honest_stream, check_restore_refusals, check_restore_stream,
                                check_roots_at_every_m, check_size, check_tamperings)
from ballot_model import STREAMS
from registry_oracle import make_keys

pytestmark = pytest.mark.gpu

PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4


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
def test_honest_log_audits_ok(ctx, device_box, name):
    """many_blocks is the 8192-ballot stream over 2048 nullifiers: its whole-log insert spans 32 blocks"""
    assert check_honest_stream(ctx, device_box, name) == check_honest_stream(None, host_box, name)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(ctx, device_box, n):
    assert check_size(ctx, device_box, n) == check_size(None, host_box, n)


@pytest.mark.parametrize("hook", [None, "registry_row=0"], ids=["default", "one_lane"])
def test_roots_at_every_m(device_box, monkeypatch, hook):
    """the prefix roots read a tree grown by 131 appends, in the row form and in the one-lane form"""
    if hook:
        monkeypatch.setenv("QPGPU_PATHS", hook)
    else:
        monkeypatch.delenv("QPGPU_PATHS", raising=False)
    assert check_roots_at_every_m(device_box) == check_roots_at_every_m(host_box)


@pytest.mark.parametrize("hook", [None, "registry_row=0"], ids=["default", "one_lane"])
def test_each_tampering_gives_its_reason_and_witness(ctx, device_box, monkeypatch, hook):
    if hook:
        monkeypatch.setenv("QPGPU_PATHS", hook)
    else:
        monkeypatch.delenv("QPGPU_PATHS", raising=False)
    assert check_tamperings(ctx, device_box) == check_tamperings(None, host_box)


@pytest.mark.parametrize("name", STREAMS)
def test_restore_continues_the_stream(ctx, device_box, name):
    """The device restores at every cut of every stream.  The host run beside it
    is there for the comparison of what the two paths observe at the end of the
    stream, which does not depend on the cuts: it takes the replayed cuts only
    (a subsample for many_blocks alone; test_ballot_audit.py runs every cut of
    it on the host path, which takes a minute and a half there)."""
    assert check_restore_stream(ctx, device_box, name) == check_restore_stream(None, host_box, name, every_cut=False)


@pytest.mark.parametrize("name", STREAMS)
def test_restore_across_paths(ctx, device_box, name):
    """host-restored from a device box's entries, and the reverse.  At the replayed
    cuts only, a subsample for many_blocks alone (18 of its 1171 cuts): the host
    half of every cut of it is test_ballot_audit.py's minute and a half again,
    and the entries a restore reads are equal across the paths by
    test_gpu_ballot_box.py, whichever box published them."""
    a = check_restore_stream(None, host_box, name, entries_factory=device_box, every_cut=False)
    b = check_restore_stream(ctx, device_box, name, entries_factory=host_box, every_cut=False)
    assert a == b


def test_restore_refusals(ctx, device_box):
    check_restore_refusals(ctx, device_box)


def test_voting_proofs_to_audit_and_restore(ctx):
    import qp_wormhole
    from qp_wormhole import BallotBox, VoterRegistry, WormholeVerifier, audit_log
    from qp_wormhole.prover import _verifier_only
    keys = make_keys(5, 6)
    com = [VoterRegistry.commitment(k) for k in keys]
    circ = qp_wormhole.Circuit.voting()
    prover = qp_wormhole.Prover(ctx, circ, 7)
    reg = VoterRegistry.from_commitments(ctx, com)
    ver = box = again = None
    auditor = qp_wormhole.Context(0)  # a fresh context that never saw the box
    try:
        votes = [True, False, True, True, False]
        inputs = [reg.inputs_for(keys[i], i, PROPOSAL, votes[i]) for i in range(5)]
        inputs.append(reg.inputs_for(keys[2], 2, PROPOSAL, not votes[2]))  # voter 2 again, the other vote
        proofs = prover.prove_inputs(inputs)
        ver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=16)
        box = BallotBox(ctx, PROPOSAL, [list(reg.root)], verifier=ver)
        assert [r.status for r in box.cast(proofs[:4])] == [0, 0, 0, 0]
        early = box.commit_log()
        assert [r.status for r in box.cast(proofs[4:5])] == [0]
        # what the operator publishes
        entries, (root, n), tally = box.entries(), box.commit_log(), box.tally
        assert n == 5 and tally == (3, 2) and box.root_at(4) == early[0]
        rep = audit_log(auditor, entries, root=root, tally=tally, commitments=[early])
        assert rep == audit_log(None, entries, root=root, tally=tally, commitments=[early])
        assert (rep.status, rep.root, rep.yes, rep.no, rep.counted) == (0, root, 3, 2, 5)
        box.free()
        box = None
        # the operator's process died: a new box from the published log counts on
        again = BallotBox.restore(auditor, PROPOSAL, [list(reg.root)], entries, verifier=ver, root=root)
        assert (again.cast_count, again.admitted, again.tally, again.commit_log()) == (5, 5, tally, (root, n))
        res = again.cast(proofs[5:])
        assert [(r.status, r.number, r.first) for r in res] == [(6, 5, 2)]  # the double vote is reported as double
        assert again.tally == tally and again.admitted == 6 and again.root_at(5) == root
    finally:
        for b in (box, again):
            if b is not None:
                b.free()
        if ver is not None:
            ver.close()
        reg.free()
        prover.free()
        circ.free()
        auditor.close()
