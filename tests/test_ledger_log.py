"""The transfer ledger's log commitment, receipts and the audit of a published
log on the host path (ctx = None), against the model of ledger_log_model.py.
The device tests (test_gpu_ledger_log.py) run the same cases and hold them
equal to these, result for result."""
import pytest

from ledger_log_model import (SIZES, check_big_totals, check_counted_double_spend, check_honest_stream,
                              check_leaf_edges, check_receipt_rules, check_roots_at_every_m, check_size,
                              check_tamperings, run_commit_stream)
from ledger_model import STREAMS


def host_ledger(roots, padding, capacity):
    from qp_wormhole import WormholeLedger
    return WormholeLedger(None, roots, padding=padding, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_commit_streams(name):
    """batchings 7 and whole commit after every batch (a reserve in between leaves the root unchanged),
    64 commits once at the end; the three final commitments and receipts are equal"""
    finals = [run_commit_stream(host_ledger, name, batching, every)
              for batching, every in ((7, True), (None, True), (64, False))]
    assert finals[0] == finals[1] == finals[2]
    assert (finals[0][1] == 0) == (name == "rejected_only")


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_promoted_nodes(n):
    check_size(host_ledger, n)


def test_leaf_edge_values():
    check_leaf_edges(host_ledger)


def test_receipt_rules():
    check_receipt_rules(host_ledger)


def test_roots_at_every_m():
    check_roots_at_every_m(host_ledger)


@pytest.mark.parametrize("name", STREAMS)
def test_audit_honest_streams(name):
    rep = check_honest_stream(None, host_ledger, name)
    assert (rep is None) == (name == "rejected_only")


def test_audit_tamperings():
    check_tamperings(None, host_ledger)


def test_audit_counted_double_spend():
    check_counted_double_spend(None, host_ledger)


def test_audit_totals_beyond_2_128():
    check_big_totals(None, host_ledger)
