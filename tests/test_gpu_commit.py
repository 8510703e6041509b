"""GPU parity: NTT/LDE, Poseidon and PolynomialBatch commitments (HIP via the
C ABI) against the CPU oracle, bit-exact.  SURVEY.md section 8 rows a4-a7."""
import numpy as np
import pytest

from edge_values import bitrev_perm, constant_columns, edge_cycle
from oracle_lib import P, commit_values, lib as olib

pytestmark = pytest.mark.gpu

G = 0xC65C18B67785D900


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def rand_felts(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def test_poseidon_permute(ctx):
    """Every state of a 4096-state batch (random, zero, all p-1, unit lanes,
    small values) equals the oracle's plain-round permutation: exercises the
    device's sparse, grouped partial rounds and their accumulator bounds."""
    import qp_wormhole
    rng = np.random.default_rng(10)
    states = rand_felts(rng, 4096, 12)
    states[0] = 0
    states[1] = P - 1
    for i in range(12):
        states[2 + i] = 0
        states[2 + i, i] = 1
        states[14 + i] = P - 1
        states[14 + i, i] = 0
    states[26:40] = rng.integers(0, 4, size=(14, 12), dtype=np.uint64)
    states[40:60] = P - 1 - rng.integers(0, 2**32, size=(20, 12), dtype=np.uint64)
    got = qp_wormhole.poseidon_permute(ctx, states)
    want = states.copy()
    for i in range(len(want)):
        olib().ora_permute(want[i])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, bad[:10]


# 15, 16: beyond one workgroup's LDS (HBM levels + 2^14-point LDS blocks)
@pytest.mark.parametrize("log_n", [1, 3, 8, 10, 13, 14, 15, 16])
def test_ifft(ctx, log_n):
    import qp_wormhole
    rng = np.random.default_rng(log_n)
    v = rand_felts(rng, 3, 1 << log_n)
    got = qp_wormhole.ifft(ctx, v)
    for c in range(3):
        e = v[c].copy()
        olib().ora_ifft(e, log_n)
        assert (got[c] == e).all()


@pytest.mark.parametrize("log_n,rate_bits", [(2, 1), (5, 3), (10, 3), (13, 3), (12, 4), (11, 1), (11, 2), (13, 1), (10, 4), (14, 2),
                                            (15, 3), (16, 2), (15, 1)])
def test_lde_leaf_order(ctx, log_n, rate_bits):
    import qp_wormhole
    rng = np.random.default_rng(100 + log_n)
    c = rand_felts(rng, 2, 1 << log_n)
    got = qp_wormhole.lde(ctx, c, rate_bits)
    logN = log_n + rate_bits
    rev = np.array([int(format(i, f"0{logN}b")[::-1], 2) for i in range(1 << logN)])
    for k in range(2):
        e = np.zeros(1 << logN, np.uint64)
        olib().ora_lde(c[k], log_n, rate_bits, G, e)
        assert (got[k] == e[rev]).all()


@pytest.mark.parametrize("npolys,log_n,rate_bits,cap_h,nsalt", [
    (1, 6, 3, 2, 0),     # leaf width 1 -> hash_or_noop pads
    (4, 6, 3, 0, 0),     # width 4 noop, cap height 0
    (5, 7, 3, 4, 0),     # width 5 -> one permutation
    (16, 8, 3, 4, 4),    # salted
    (20, 9, 3, 4, 0),
    (84, 8, 3, 4, 0),    # constants||sigmas width
    (135, 8, 3, 4, 4),   # salted wires width 139
    (2, 3, 1, 4, 0),     # cap_h = log N: the tree is all cap, depth 0, no siblings to gather
])
def test_commit_values_parity(ctx, npolys, log_n, rate_bits, cap_h, nsalt):
    import qp_wormhole
    rng = np.random.default_rng(npolys * 1000 + log_n)
    vals = rand_felts(rng, npolys, 1 << log_n)
    salt = rand_felts(rng, 1 << (log_n + rate_bits), nsalt) if nsalt else None
    coeffs_o, leaves_o, cap_o = commit_values(vals, log_n, rate_bits, cap_h, salt=salt, want_leaves=True)
    b = qp_wormhole.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h, salt=salt)
    assert (b.coeffs == coeffs_o).all()
    assert (b.cap == cap_o).all()
    assert (b.lde() == leaves_o[:, :npolys].T).all()
    # openings: leaves + Merkle paths against the oracle's tree
    N = 1 << (log_n + rate_bits)
    idx = np.array([0, 1, N - 1, N // 2, 12345 % N], np.uint32)
    leaves, sibs = b.open(idx)
    assert (leaves == leaves_o[idx]).all()
    depth = log_n + rate_bits - cap_h
    cap2 = np.zeros(((1 << cap_h), 4), np.uint64)
    sib_o = np.zeros((len(idx), depth, 4), np.uint64)
    olib().ora_merkle(np.ascontiguousarray(leaves_o), log_n + rate_bits, leaves_o.shape[1], cap_h, cap2,
                      idx.astype(np.uint64), len(idx), sib_o)
    assert (cap2 == cap_o).all()
    assert sibs.shape == sib_o.shape and (sibs == sib_o).all()
    b.free()


def lde_oracle_leaf_order(c, log_n, rate_bits):
    logN = log_n + rate_bits
    rev = bitrev_perm(logN)
    want = np.zeros((len(c), 1 << logN), np.uint64)
    e = np.zeros(1 << logN, np.uint64)
    for k in range(len(c)):
        olib().ora_lde(np.ascontiguousarray(c[k]), log_n, rate_bits, G, e)
        want[k] = e[rev]
    return want


@pytest.mark.parametrize("log_n,rate_bits", [(ln, r) for ln in range(10, 15) for r in range(1, 5)])
def test_lde_cosets_kernel(ctx, monkeypatch, log_n, rate_bits):
    """k_lde_cosets<LOG_T> (one workgroup per column walking its cosets), which
    the heuristic picks from 256 columns on, at every size and rate it is built
    for: each LOG_T with its tail_group<G> store loop, each rate's pre-twist
    (ptw) and merged-twiddle (mtw) tables.  Path hook lde_few=0 forces it for
    three columns: uniform, all p-1, a cycle through the canonical edge values."""
    import qp_wormhole
    assert log_n + rate_bits <= 18
    n = 1 << log_n
    rng = np.random.default_rng(1000 * log_n + rate_bits)
    c = np.stack([rand_felts(rng, n), np.full(n, P - 1, np.uint64), edge_cycle(n)])
    monkeypatch.delenv("QPGPU_PATHS", raising=False)
    per_coset = qp_wormhole.lde(ctx, c, rate_bits)  # 3 columns: k_lde
    monkeypatch.setenv("QPGPU_PATHS", "lde_few=0")
    fused = qp_wormhole.lde(ctx, c, rate_bits)
    want = lde_oracle_leaf_order(c, log_n, rate_bits)
    assert (fused == want).all(), np.argwhere(fused != want)[:4]
    assert (fused == per_coset).all()


def test_lde_cosets_kernel_by_heuristic(ctx, monkeypatch):
    """256 columns reach the fused kernel through the heuristic itself."""
    import qp_wormhole
    log_n, rate_bits = 10, 1
    rng = np.random.default_rng(256)
    c = rand_felts(rng, 256, 1 << log_n)
    c[1] = P - 1
    c[2] = edge_cycle(1 << log_n)
    monkeypatch.delenv("QPGPU_PATHS", raising=False)
    got = qp_wormhole.lde(ctx, c, rate_bits)
    want = lde_oracle_leaf_order(c, log_n, rate_bits)
    assert (got == want).all(), np.argwhere(got != want)[:4]
    monkeypatch.setenv("QPGPU_PATHS", "lde_few=1000000")  # the same columns through k_lde
    assert (qp_wormhole.lde(ctx, c, rate_bits) == want).all()


W_2_32 = 7277203076849721926  # plonky2's generator of the 2^32-th roots of unity (field.h TWO_ADIC_GEN)


def structured_columns(n):
    """Columns that keep the butterflies' inputs on the edges of the field."""
    i = np.arange(n, dtype=np.uint64)
    even, top = i % np.uint64(2) == 0, np.uint64(P - 1)
    cols = [np.full(n, P - 1, np.uint64), np.where(even, top, np.uint64(0)), np.where(even, np.uint64(0), top),
            np.where(even, top, np.uint64(1))]
    for at in (0, n // 2, n - 1):
        col = np.zeros(n, np.uint64)
        col[at] = P - 1
        cols.append(col)
    cols += [np.full(n, 2**32 - 1, np.uint64), np.full(n, P - 2**32, np.uint64), np.uint64(P - 1) - i]
    return np.stack(cols)


def dft_ifft(v, log_n):
    """c_k = n^-1 sum_j v_j w^(-jk), Python integers."""
    n = 1 << log_n
    w_inv = pow(pow(W_2_32, 1 << (32 - log_n), P), P - 2, P)
    n_inv = pow(n, P - 2, P)
    pw = [pow(w_inv, e, P) for e in range(n)]
    return [n_inv * sum(v[j] * pw[j * k % n] for j in range(n)) % P for k in range(n)]


def dft_lde(c, log_n, rate_bits):
    """The coefficients c evaluated on the coset G <w_N>, in bit-reversed (leaf) order."""
    n, logN = 1 << log_n, log_n + rate_bits
    N = 1 << logN
    w = pow(W_2_32, 1 << (32 - logN), P)
    pw = [pow(w, e, P) for e in range(N)]
    cg = [c[j] * pow(G, j, P) % P for j in range(n)]
    ev = [sum(cg[j] * pw[i * j % N] for j in range(n)) % P for i in range(N)]
    return [ev[r] for r in bitrev_perm(logN)]


@pytest.mark.parametrize("log_n,rate_bits", [(1, 3), (2, 3), (3, 3), (4, 3), (5, 3), (6, 3),
                                             (10, 3), (13, 3), (14, 3), (15, 3), (16, 2)])
def test_transforms_edge_values(ctx, log_n, rate_bits):
    """qp_ifft and qp_lde on edge-valued columns.  log_n <= 6: against an O(n^2)
    DFT in Python integers; each of these sizes ends in a different
    tail<LOGS> / pass32 combination, and up to n = 16 the first butterfly stage
    acts on the raw inputs, so add4 / sub4 / mul_pow2 see the edge values
    themselves.  Larger sizes against the oracle; 15 and 16 run the HBM-level
    kernels k_dif_level, k_bitrev_scale and k_coset_scale."""
    import qp_wormhole
    cols = structured_columns(1 << log_n)
    got = qp_wormhole.ifft(ctx, cols)
    if log_n <= 6:
        ints = [[int(x) for x in col] for col in cols]
        for k, col in enumerate(ints):
            assert [int(x) for x in got[k]] == dft_ifft(col, log_n), ("ifft", k)
        for rb in (1, rate_bits):
            got = qp_wormhole.lde(ctx, cols, rb)
            for k, col in enumerate(ints):
                assert [int(x) for x in got[k]] == dft_lde(col, log_n, rb), ("lde", rb, k)
        return
    for k in range(len(cols)):
        e = cols[k].copy()
        olib().ora_ifft(e, log_n)
        assert (got[k] == e).all(), ("ifft", k)
    got = qp_wormhole.lde(ctx, cols, rate_bits)
    want = lde_oracle_leaf_order(cols, log_n, rate_bits)
    assert (got == want).all(), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("npolys", [5, 20, 135])
def test_commit_constant_columns(ctx, npolys):
    """Every column constant over H at a canonical edge value: its LDE is that
    constant, so every leaf the leaf-hash kernels (widths 5, 20, 135) absorb is
    made of edge values."""
    import qp_wormhole
    log_n, rate_bits, cap_h = 6, 3, 2
    vals = constant_columns(npolys, 1 << log_n)
    coeffs_o, leaves_o, cap_o = commit_values(vals, log_n, rate_bits, cap_h, want_leaves=True)
    assert (leaves_o == vals[:, 0]).all()  # the leaves are the edge values
    b = qp_wormhole.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h)
    assert (b.coeffs == coeffs_o).all()
    assert (b.cap == cap_o).all()
    N = 1 << (log_n + rate_bits)
    idx = np.array([0, N - 1], np.uint32)
    leaves, sibs = b.open(idx)
    assert (leaves == leaves_o[idx]).all()
    depth = log_n + rate_bits - cap_h
    cap2 = np.zeros(((1 << cap_h), 4), np.uint64)
    sib_o = np.zeros((len(idx), depth, 4), np.uint64)
    olib().ora_merkle(np.ascontiguousarray(leaves_o), log_n + rate_bits, leaves_o.shape[1], cap_h, cap2,
                      idx.astype(np.uint64), len(idx), sib_o)
    assert (cap2 == cap_o).all()
    assert (sibs == sib_o).all()
    b.free()


def test_commit_coeffs_parity(ctx):
    import qp_wormhole
    rng = np.random.default_rng(7)
    co = rand_felts(rng, 16, 1 << 9)
    _, _, cap_o = commit_values(co, 9, 3, 4, from_coeffs=True)
    b = qp_wormhole.PolynomialBatch.from_coeffs(ctx, co, 3, 4)
    assert (b.cap == cap_o).all()
    b.free()


def test_commit_full_size_wires(ctx):
    """Full Wormhole wires shape (135 x 2^13, blowup 8, cap 16) bit-exact vs the oracle."""
    import qp_wormhole
    rng = np.random.default_rng(2024)
    vals = rand_felts(rng, 135, 1 << 13)
    coeffs_o, _, cap_o = commit_values(vals, 13, 3, 4)
    b = qp_wormhole.PolynomialBatch.from_values(ctx, vals, 3, 4)
    assert (b.coeffs == coeffs_o).all()
    assert (b.cap == cap_o).all()
    b.free()


def test_bad_shape_is_an_error(ctx):
    """Beyond the twiddle tables (2^16 values at rate 3 = 2^19 points > 2^18):
    an error with the reason, not a wrong result."""
    import qp_wormhole
    with pytest.raises(qp_wormhole.QpError):
        qp_wormhole.PolynomialBatch.from_values(ctx, np.zeros((2, 1 << 16), np.uint64), 3, 4)
