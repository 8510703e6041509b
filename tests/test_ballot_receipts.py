"""The ballot box's log commitment on the host path (ctx None; csrc/ballot_log.h
through qp_ballot_box_find / _commit_log / _receipts / qp_ballot_receipt_check):
every stream of ballot_model.py against the model of ballot_receipt_model.py
(the oracle's hash_no_pad, the registry model's level loop and path), the tree
sizes around the promoted nodes and the fold bound, find, and the receipt
rules."""
import pytest

from ballot_receipt_model import (SIZES, STREAMS, check_find, check_receipt_rules, check_size, run_commit_stream)


def host_box(proposal, roots, capacity):
    from qp_wormhole import BallotBox
    return BallotBox(None, proposal, roots, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_root_matches_model_incrementally_and_from_scratch(name):
    """batchings 7 and whole commit after every batch (incremental appends, each
    held to the model's root at that n); batching 64 commits once at the end
    (from scratch); the final commitment is the same under all three"""
    finals = []
    for batching, every in ((7, True), (None, True), (64, False)):
        root, n, model, logm, box = run_commit_stream(host_box, name, batching, every)
        box.free()
        finals.append((root, n))
    assert finals[0] == finals[1] == finals[2]


def test_stream_shapes_are_what_their_names_say():
    root, n, model, logm, box = run_commit_stream(host_box, "one_nullifier", 64, False)
    box.free()
    assert n == 64 and sum(e[2] for e in model.log) == 1  # the leaf level is exactly the fold bound
    root, n, model, logm, box = run_commit_stream(host_box, "screened", None, True)
    box.free()
    assert (model.cast, n) == (16, 6)  # rejected ballots take no leaf
    root, n, model, logm, box = run_commit_stream(host_box, "many_blocks", 64, False)
    box.free()
    assert n == 8192


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_promoted_nodes(n):
    check_size(host_box, n)


def test_find():
    check_find(host_box)


def test_receipt_rules():
    check_receipt_rules(host_box)


def test_exports():
    import qp_wormhole
    assert "BallotReceipt" in qp_wormhole.__all__ and qp_wormhole.BallotReceipt.__module__ == "qp_wormhole.ballot"
    assert qp_wormhole.BallotReceipt._fields == ("nullifier", "number", "vote", "counted", "seq", "siblings",
                                                 "path_bits", "depth", "root", "n")
