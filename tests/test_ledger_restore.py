"""Reopening a transfer ledger from its published log (qp_ledger_restore) and
payout rounds (qp_ledger_payouts_between, qp_ledger_log_payouts_between) on the
host path (ctx = None), against the model of ledger_restore_model.py.  The
device tests (test_gpu_ledger_restore.py) run the same cases and hold them equal
to these, result for result."""
import pytest

from ledger_model import STREAMS
from ledger_restore_model import (EDGE_SIZES, check_block_edges, check_restore_refusals, check_restore_stream,
                                  check_round_big, check_round_identities, check_round_ranges, check_round_sizing)


def host_ledger(roots, padding, capacity):
    from qp_wormhole import WormholeLedger
    return WormholeLedger(None, roots, padding=padding, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_restore_at_the_cuts(name):
    check_restore_stream(None, host_ledger, name)


@pytest.mark.parametrize("n", EDGE_SIZES)
def test_restore_block_edges(n):
    check_block_edges(None, host_ledger, n)


def test_restore_refusals():
    check_restore_refusals(None, host_ledger)


@pytest.mark.parametrize("name", STREAMS)
def test_round_identities(name):
    check_round_identities(None, host_ledger, name)


def test_round_ranges():
    check_round_ranges(None, host_ledger)


def test_round_totals_beyond_2_128():
    check_round_big(None, host_ledger)


def test_round_sizing_and_cap():
    check_round_sizing(None, host_ledger)
