"""The audit of a published ballot log, prefix roots and restore on the host
path (ctx None; csrc/ballot_audit.h through qp_ballot_log_audit,
qp_ballot_box_roots_at and qp_ballot_box_restore) against the model of
ballot_audit_model.py.  tests/test_gpu_ballot_audit.py repeats every case on
the device."""
import pytest

from ballot_audit_model import (SIZES, check_honest_stream, check_restore_refusals, check_restore_stream,
                                check_roots_at_every_m, check_size, check_tamperings)
from ballot_model import STREAMS


def host_box(proposal, roots, capacity):
    from qp_wormhole import BallotBox
    return BallotBox(None, proposal, roots, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_honest_log_audits_ok(name):
    check_honest_stream(None, host_box, name)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    """a lone leaf, promoted nodes at and above the leaf level, one node past
    ACC_FOLD_MAX, a neighbour compare across a 256-lane block edge"""
    check_size(None, host_box, n)


def test_roots_at_every_m():
    check_roots_at_every_m(host_box)


def test_each_tampering_gives_its_reason_and_witness():
    check_tamperings(None, host_box)


@pytest.mark.parametrize("name", STREAMS)
def test_restore_continues_the_stream(name):
    check_restore_stream(None, host_box, name)


def test_restore_refusals():
    check_restore_refusals(None, host_box)


def test_exports():
    import qp_wormhole
    for name in ("audit_log", "AuditReport", "AUDIT_STATUS_TEXT"):
        assert name in qp_wormhole.__all__
    assert qp_wormhole.AuditReport._fields == ("status", "witness", "first", "root", "yes", "no", "counted")
    assert len(qp_wormhole.AUDIT_STATUS_TEXT) == 7
    assert all(hasattr(qp_wormhole.BallotBox, m) for m in ("root_at", "roots_at", "restore"))
