"""The seams that take the last host-side polynomial work of INTEGRATION.md
binding A to the device: qp_partial_products_and_zs, qp_opening_set /
qp_batch_eval_ext and qp_fri_initial_poly.  Each against the CPU oracle's
stand-in (or a plain-integer reference for shapes no circuit has), exact
equality throughout; then plonky2's prove() composed from the seams alone
(tests/seam_stage_prover.py) against the whole-circuit prover's bytes; then the
calls outside the limits, which must come back as QP_ERR_ARG."""
import numpy as np
import pytest

import wormhole_inputs as WI
from oracle_lib import P
from seam_prover import _bind, evals_ext
from seam_stage_prover import k_is, prove, ref_partial_products_and_zs, root_of_unity

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(0x5EA5)


def felts(*shape):
    return RNG.integers(0, P, size=shape, dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def _voting():
    import qp_wormhole
    from qp_wormhole.synthetic import synthetic_vote_inputs
    circ = qp_wormhole.Circuit.voting()
    return circ, circ.commit(synthetic_vote_inputs(3))


def _wormhole(zk=False):
    import qp_wormhole
    circ = qp_wormhole.Circuit.wormhole(zero_knowledge=zk)
    return circ, circ.commit(WI.test_inputs())


def _aggregation15():
    """the circuit of test_seam_composed_degree15_aggregation_proof"""
    import qp_wormhole
    from current_circuit_vd import current_circuit_verifier_data
    from oracle_lib import golden
    from test_oracle_golden import current_common_bytes
    cb = current_common_bytes()
    vd = current_circuit_verifier_data(cb)[0]
    vo = vd[:len(vd) - len(cb)]
    leaves = [golden("dummy_proof.bin"), golden("dummy_proof_zk.bin")]
    circ = qp_wormhole.Circuit.aggregation(cb, 5)
    assert circ.degree_bits == 15
    return circ, circ.commit_proofs(vo, [leaves[i % 2] for i in range(5)])


# ---- 1. partial products and Z ------------------------------------------------

@pytest.mark.parametrize("make, log_n", [(_voting, 8), (_wormhole, 13)])
def test_partial_products_of_real_witnesses(ctx, make, log_n):
    import qp_wormhole as q
    circ, w = make()
    assert circ.degree_bits == log_n
    g = q.gate_desc(circ)
    R, qdf, nc = g.num_routed_wires, g.quotient_degree_factor, g.num_challenges
    cs_vals, wires, common = circ.constants_sigmas(), w.wires(), circ.common_data()
    betas, gammas = felts(nc), felts(nc)
    want = np.zeros((nc * ((R + qdf - 1) // qdf), circ.n), np.uint64)
    assert _bind().ora_zs_values(common, len(common), cs_vals, wires, betas, gammas, want) == 0
    perm = q.PermutationData(ctx, cs_vals[-R:], k_is(R))
    got = perm.partial_products_and_zs(wires, qdf, betas, gammas)
    perm.free()
    assert got.shape == want.shape and np.array_equal(got, want)


def _random_pp_case(ctx, log_n, R, qdf, challenges):
    """random nonzero wires and sigmas against the plain-integer reference; challenges:
    list of (betas, gammas), one call each"""
    import qp_wormhole as q
    n = 1 << log_n
    wires = RNG.integers(1, P, size=(R + 2, n), dtype=np.uint64)  # two unrouted columns the call must not read
    sigmas = RNG.integers(1, P, size=(R, n), dtype=np.uint64)
    perm = q.PermutationData(ctx, sigmas, k_is(R))
    for betas, gammas in challenges:
        want, dens_ok = ref_partial_products_and_zs(wires.tolist(), sigmas.tolist(), k_is(R).tolist(), qdf, betas,
                                                    gammas)
        assert dens_ok, "the test's own inputs: no denominator may be zero"
        got = perm.partial_products_and_zs(wires, qdf, betas, gammas)
        assert got.shape == want.shape and np.array_equal(got, want), (log_n, R, qdf, betas, gammas)
    perm.free()


def _edge_challenges():
    r = [int(x) for x in felts(4)]
    # (random, random), (beta = 0), then (gamma = 0), (beta = gamma = p - 1)
    return [([r[0], 0], [r[1], r[2]]), ([r[3], P - 1], [0, P - 1])]


def test_partial_products_leaf_shape_random(ctx):
    """(R, qdf) = (80, 8), two challenges: k_pp_rows_t<80, 8>, the edge challenges included"""
    _random_pp_case(ctx, 6, 80, 8, _edge_challenges())


def test_partial_products_short_last_chunk(ctx):
    """(R, qdf) = (7, 4): a last chunk of 3, the generic k_pp_rows; also one challenge alone"""
    _random_pp_case(ctx, 6, 7, 4, _edge_challenges() + [([int(felts(1)[0])], [int(felts(1)[0])])])


def test_partial_products_above_the_lds_scan(ctx):
    """n = 2^15 > 2^LDS_LOG_MAX: k_z_scan's HBM form; one chunk, so no partial products"""
    r = [int(x) for x in felts(3)]
    _random_pp_case(ctx, 15, 8, 8, [([r[0], 0], [r[1], r[2]])])


# ---- 2. openings ----------------------------------------------------------------

def _batches(ctx, log_n, counts, rate_bits=3, cap_h=0):
    import qp_wormhole as q
    return [q.PolynomialBatch.from_coeffs(ctx, felts(k, 1 << log_n), rate_bits, cap_h) for k in counts]


def _ext_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _want_opening_set(bs, nc, zeta, log_n):
    zn = _ext_mul(zeta, (root_of_unity(log_n), 0))
    return np.concatenate([evals_ext(b.coeffs, zeta) for b in bs] + [evals_ext(bs[2].coeffs[:nc], zn)])


@pytest.mark.parametrize("log_n", [8, 13])
def test_opening_set_of_the_leaf_column_counts(ctx, log_n, monkeypatch):
    import qp_wormhole as q
    bs = _batches(ctx, log_n, (84, 135, 20, 16))
    zeta = tuple(int(x) for x in felts(2))
    want = _want_opening_set(bs, 2, zeta, log_n)
    got = q.opening_set(ctx, *bs, 2, zeta)
    assert got.shape == (257, 2) and np.array_equal(got, want)
    # one block per column group instead of coefficient slices: the same bytes
    monkeypatch.setenv("QPGPU_PATHS", "open_slices=1")
    one = q.opening_set(ctx, *bs, 2, zeta)
    monkeypatch.delenv("QPGPU_PATHS")
    assert np.array_equal(one, got)
    for b in bs:
        b.free()


@pytest.mark.parametrize("log_n", [1, 5, 6])
def test_eval_ext_windows_and_edge_points(ctx, log_n):
    (b,) = _batches(ctx, log_n, (21,))
    pts = [tuple(int(x) for x in felts(2)), (0, 1), (P - 1, P - 1), (1, 0), (0, 0)]
    for first, npolys in [(0, None), (3, 13), (7, 1), (20, 1), (5, 15)]:  # windows off the multiples of OPEN_PB = 8
        k = b.npolys - first if npolys is None else npolys
        got = b.eval_ext(pts, first, npolys)
        assert got.shape == (len(pts), k, 2)
        for i, pt in enumerate(pts):
            assert np.array_equal(got[i], evals_ext(b.coeffs[first:first + k], pt)), (log_n, first, npolys, pt)
    b.free()


def test_eval_ext_wider_than_one_row(ctx):
    """more polynomials than one launch's result row (260) and several points"""
    (b,) = _batches(ctx, 6, (263,))
    pts = [tuple(int(x) for x in felts(2)) for _ in range(3)]
    got = b.eval_ext(pts)
    for i, pt in enumerate(pts):
        assert np.array_equal(got[i], evals_ext(b.coeffs, pt))
    b.free()


# ---- 3. the initial FRI polynomial ---------------------------------------------------

def _want_fri_initial(bs, nc, alpha, zeta, log_n):
    zn = _ext_mul(zeta, (root_of_unity(log_n), 0))
    fin = np.zeros((1 << log_n, 2), np.uint64)
    _bind().ora_fri_initial(bs[0].coeffs, bs[0].npolys, bs[1].coeffs, bs[1].npolys, bs[2].coeffs, bs[2].npolys,
                            bs[3].coeffs, bs[3].npolys, nc, log_n, np.array(alpha, np.uint64),
                            np.array(zeta, np.uint64), np.array(zn, np.uint64), fin)
    return np.ascontiguousarray(fin.T)


@pytest.mark.parametrize("log_n, counts, nc", [
    (6, (3, 5, 4, 2), 1),            # the thread-count floor (8 threads); one challenge
    (6, (3, 5, 4, 2), 2),
    (8, (84, 135, 20, 16), 2),       # the voting circuit's columns
    (13, (3, 5, 4, 2), 2),           # 8 values per thread at 1024 threads
    (14, (3, 5, 4, 2), 2),           # 16 per thread: the last size of k_fri_divide<16>
    (15, (3, 5, 4, 2), 2)])          # 32 per thread: k_fri_divide<64>
def test_fri_initial_poly(ctx, log_n, counts, nc):
    import qp_wormhole as q
    bs = _batches(ctx, log_n, counts)
    alpha, zeta = tuple(int(x) for x in felts(2)), tuple(int(x) for x in felts(2))
    want = _want_fri_initial(bs, nc, alpha, zeta, log_n)
    got = q.fri_initial_poly(ctx, *bs, nc, alpha, zeta)
    assert got.shape == (2, 1 << log_n) and np.array_equal(got, want)
    for b in bs:
        b.free()


# ---- 4. composition ------------------------------------------------------------------

@pytest.mark.parametrize("make", [_voting, lambda: _wormhole(False), lambda: _wormhole(True), _aggregation15],
                         ids=["voting", "wormhole", "wormhole_zk", "aggregation_2^15"])
def test_prove_composed_from_the_seams_alone(ctx, make):
    """plonky2's prove() with the oracle supplying only the transcript's Poseidon: the
    whole-circuit prover's bytes, and they verify."""
    import qp_wormhole as q
    circ, w = make()
    seam = prove(ctx, circ, w.wires(), w.public_inputs(), stages="seam")
    whole = q.Prover(ctx, circ, 1)
    assert seam == whole.prove_witnesses([w])[0]
    vd, cb = whole.verifier_data(), circ.common_data()
    whole.free()
    v = q.WormholeVerifier.new_from_bytes(vd[:len(vd) - len(cb)], cb, device=None, max_batch=1)
    assert v.verify_batch([seam]) == [0]
    v.close()


# ---- 5. refusals ---------------------------------------------------------------------

def _refused(fn, *a):
    import qp_wormhole as q
    with pytest.raises(q.QpError) as e:
        fn(*a)
    assert e.value.code == 1, e.value  # QP_ERR_ARG


def test_calls_outside_the_limits_are_refused(ctx):
    import qp_wormhole as q
    zeta, alpha = (3, 5), (11, 13)
    good = _batches(ctx, 6, (100, 100, 30, 28))  # 258 + 2 = 260 openings: the most one call takes

    def both(bs, nc=2, z=zeta):
        _refused(q.opening_set, ctx, *bs, nc, z)
        _refused(q.fri_initial_poly, ctx, *bs, nc, alpha, z)

    # batches of different log_n, each position
    (other_n,) = _batches(ctx, 7, (4,))
    for i in range(4):
        both(good[:i] + [other_n] + good[i + 1:])
    # a salted batch
    salted = q.PolynomialBatch.from_coeffs(ctx, felts(4, 64), 3, 0, salt=felts(512, 4))
    both([good[0], salted, good[2], good[3]])
    # a batch of another context
    ctx2 = q.Context(0)
    (foreign,) = _batches(ctx2, 6, (4,))
    both([good[0], good[1], good[2], foreign])
    # n = 2^5 and n = 2^16
    for log_n in (5, 16):
        small = _batches(ctx, log_n, (1, 1, 2, 1), rate_bits=2)
        both(small)
        _refused(q.PermutationData, ctx, felts(2, 1 << log_n), k_is(2))
        for b in small:
            b.free()
    # 261 openings
    (one_more,) = _batches(ctx, 6, (29,))
    _refused(q.opening_set, ctx, good[0], good[1], good[2], one_more, 2, zeta)
    # zeta = 0, zeta in the subgroup
    both(good, z=(0, 0))
    both(good, z=(pow(root_of_unity(6), 3, P), 0))
    both(good, z=(1, 0))
    # three challenges; fewer Zs than challenges
    both(good, nc=3)
    (one_z,) = _batches(ctx, 6, (1,))
    both([good[0], good[1], one_z, good[3]])
    # the permutation seam: three challenges, more than 16 chunks, a zero quotient degree factor
    perm = q.PermutationData(ctx, felts(80, 64), k_is(80))
    w = felts(80, 64)
    _refused(perm.partial_products_and_zs, w, 8, [1, 2, 3], [4, 5, 6])
    _refused(perm.partial_products_and_zs, w, 4, [1, 2], [4, 5])
    with pytest.raises((q.QpError, ValueError)):
        perm.partial_products_and_zs(w, 0, [1, 2], [4, 5])
    # windows outside a batch
    with pytest.raises((q.QpError, ValueError)):
        good[3].eval_ext([zeta], 20, 9)
    rc = q.lib().qp_batch_eval_ext(good[3].h, 20, 9, np.array(zeta, np.uint64), 1, np.zeros(18, np.uint64))
    assert rc == 1
    # the same context still works: the widest legal opening set, the FRI polynomial, the products
    got = q.opening_set(ctx, *good, 2, zeta)
    assert got.shape == (260, 2) and np.array_equal(got, _want_opening_set(good, 2, zeta, 6))
    assert np.array_equal(q.fri_initial_poly(ctx, *good, 2, alpha, zeta), _want_fri_initial(good, 2, alpha, zeta, 6))
    assert perm.partial_products_and_zs(w, 8, [1, 2], [4, 5]).shape == (20, 64)
    perm.free()
    for b in good + [other_n, salted, foreign, one_more, one_z]:
        b.free()
    ctx2.close()
