"""pf::dense_group (poseidon_fast.h), the small-integer grouped partial rounds
of the hashing permutation, through the TEST-ONLY probe qp_debug_poseidon_op:
every group start of the shipped plan on the edge states and 2^10 uniform
states of test_gpu_poseidon_forms.state_set("u64") plus the states of
test_poseidon_dense.carry_states (y_1 and every output row take reduce_row's
carry).  Residues against Python integers, raw words against the exact al, ah
followed by m_reduce_row.  All comparisons are exact."""
import numpy as np
import pytest

import test_poseidon_dense as D
from qp_wormhole import _native as N
from test_gpu_poseidon_forms import canon_rows, check_residues

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("t0", D.STARTS)
def test_dense_group(ctx, t0):
    D.test_state_set_takes_both_carries(t0)
    s = D.group_states(t0)
    out = N.debug_poseidon_op(ctx, N.PFORM_DENSE_GROUP, s, param=t0)
    check_residues(out, [D.r_dense_group(v, t0) for v in canon_rows(s)], range(12), f"dense_group<{t0}>")
    assert (out == D.group_model(s, t0)[0]).all(), f"dense_group<{t0}>: raw result differs from the documented steps"


@gpu
def test_probe_rejects_bad_dense_group_arguments(ctx):
    import qp_wormhole
    ok = np.zeros((2, 12), np.uint64)
    for param in sorted(set(range(23)) - set(D.STARTS)) + [24, 1 << 31]:
        with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
            N.debug_poseidon_op(ctx, N.PFORM_DENSE_GROUP, ok, param=param)
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        N.debug_poseidon_op(ctx, N.PFORM_DENSE_GROUP, None, param=D.STARTS[1])
    assert N.PFORM_DENSE_GROUP == 15 and N.PFORM_COUNT == 16
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        N.debug_poseidon_op(ctx, N.PFORM_COUNT, ok)
