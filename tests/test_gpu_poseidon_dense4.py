"""pf::reduce_row_wide and pf::dense_group over the groups of up to four
(pf::TabG4, poseidon_fast.h) that the hashing permutation runs, through the
TEST-ONLY probes qp_debug_field_op and qp_debug_poseidon_op: the reduction's
raw words against its step model on the edge cross product plus 2^16 uniform
pairs; every group start of the shipped plan on the edge states and 2^10
uniform states of test_gpu_poseidon_forms.state_set("u64") plus the states of
test_poseidon_dense4.carry_states (every row takes both values of each of its
carries), residues against Python integers and raw words against the exact
al, ah followed by the row's reduction; the whole permutations on the "u64" and
"capz" state sets.  All comparisons are exact."""
import numpy as np
import pytest

import test_poseidon_dense4 as D
from qp_wormhole import _native as N
from test_gpu_poseidon_forms import canon_rows, check_residues, permuted, state_set

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@gpu
def test_reduce_row_wide(ctx):
    D.test_operand_set_covers_reachable_carry_combinations()
    a, b = D.wide_pair_set()
    out = N.debug_field_op(ctx, N.FOP_PF_REDUCE_ROW_WIDE, a, b)
    with np.errstate(over="ignore"):
        model, path = D.m_reduce_row_wide(a, b)
    assert not (path & D.U(D.WIDE_NEVER)).any()
    assert (out == model).all(), "reduce_row_wide: raw result differs from the documented steps"
    n = len(D.wide_edges()[0]) * len(D.wide_edges()[1])
    for x, y, z in zip(a[:n].tolist(), b[:n].tolist(), out[:n].tolist()):
        assert z % D.P == (x + (y << 32)) % D.P, (x, y)


@gpu
@pytest.mark.parametrize("t0", D.STARTS)
def test_dense_group4(ctx, t0):
    D.test_state_set_takes_both_values_of_every_carry(t0)
    s = D.group_states(t0)
    out = N.debug_poseidon_op(ctx, N.PFORM_DENSE_GROUP4, s, param=t0)
    G = D.header_tables()[0][t0]
    plain = [D.r_plain_partial_rounds(v, t0, G) for v in canon_rows(s)]
    check_residues(out, plain, range(12), f"dense_group<{t0}, {G}, TabG4>")
    assert (out == D.group_model(s, t0)[0]).all(), f"dense_group<{t0}, {G}, TabG4>: raw result differs from the documented steps"


@gpu
def test_permutations_on_their_state_sets(ctx):
    """pf::permute_nc and pf::permute_nc_capz<0xF> run the groups of four."""
    s = state_set("u64")[0]
    check_residues(N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, s), permuted("u64"), range(12), "permute_nc")
    z = state_set("capz")[0]
    check_residues(N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_CAPZ, z), permuted("capz"), range(4), "permute_nc_capz<0xF>")
    check_residues(N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, z), permuted("capz"), range(12), "permute_nc on capz states")
    assert D.r_permute_grouped(canon_rows(s[:1])[0]) == permuted("u64")[0]


@gpu
def test_probe_rejects_bad_dense_group4_arguments(ctx):
    import qp_wormhole
    ok = np.zeros((2, 12), np.uint64)
    for param in sorted(set(range(23)) - set(D.STARTS)) + [24, 1 << 31]:
        with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
            N.debug_poseidon_op(ctx, N.PFORM_DENSE_GROUP4, ok, param=param)
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        N.debug_poseidon_op(ctx, N.PFORM_DENSE_GROUP4, None, param=D.STARTS[1])
    assert N.PFORM_DENSE_GROUP4 == 17 and N.FOP_PF_REDUCE_ROW_WIDE == 24 and N.FOP_COUNT == 25
    for form in (N.PFORM_COUNT, N.PFORM_DENSE_GROUP4 + 1):
        with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
            N.debug_poseidon_op(ctx, form, ok)
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        N.debug_field_op(ctx, N.FOP_COUNT, np.zeros(4, np.uint64), np.zeros(4, np.uint64))
