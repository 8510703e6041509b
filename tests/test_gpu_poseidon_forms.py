"""Every device Poseidon form the production kernels instantiate, one at a
time, on edge-valued and non-canonical states.

The hashing kernels run pf:: (poseidon_fast.h) and pc:: (poseidon_coop.h):
hand-placed v_mad_u64_u32 chains on non-canonical values whose correctness
arguments are accumulator bounds.  Inside whole trees and proofs every input of
those forms is a digest or a random column, so a crossed DPP row, an OUT mask
off by a lane, a wrong CAPZ_K row or a bound that fails only when every half is
2^32 - 1 shows up as "proof bytes differ", or not at all.  Here the TEST-ONLY
probe qp_debug_poseidon_op (csrc/poseidon_probe.hip) runs one form on chosen
states and returns the raw words:

  * the references are Python integers only (the plain permutation, the MDS
    matrix, the round constants and the derive() outputs of
    tools/gen_poseidon_partial.py), never the C oracle; a CPU test composes the
    piece references in the order pf::rounds<0> applies them and requires the
    plain permutation, so the piece references are themselves pinned;
  * the states: every lane at one edge value (the values in [p, 2^64) and
    2^64 - 1 give the accumulator maxima), one edge lane among uniform lanes at
    every position, one uniform lane among 2^64 - 1 lanes, 2^10 uniform states,
    and for the pieces that fold a constant one constructed state per output
    row that takes reduce_row's carry;
  * for the MDS-type pieces the raw word must equal a restatement of the
    documented steps (the exact integer al, ah, then reduce_row's three steps,
    test_gpu_field_ops.m_reduce_row), and a CPU-side coverage condition
    requires both values of every output lane's carry in the piece's state set;
  * the 16-lane-row forms get four different states per wave with the edge
    state at each row position in turn, and state counts that leave rows and
    waves past the end.

All comparisons are exact.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from edge_values import EDGES, P
from qp_wormhole import _native as N
from test_gpu_field_ops import EDGE_VALUES, HALVES, m_mul, m_reduce_row

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
U = np.uint64
NUNIFORM = 1 << 10


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("gen_poseidon_partial",
                                                  os.path.join(ROOT, "tools", "gen_poseidon_partial.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def derived():
    return gen().derive()


def capz_k():
    """CAPZ_K[r] = RC[1][r] + sum_(j >= 8) M[r][j] sbox(RC[0][j])."""
    g = gen()
    return [(g.RC[1][r] + sum(g.M[r][j] * pow(g.RC[0][j], 7, P) for j in range(8, 12))) % P for r in range(12)]


# ---- piece references: exact integer maps on residues -------------------------

def r_sbox12(s):
    return [pow(x, 7, P) for x in s]


def r_mds(s, k=None):
    """M s + k (k = None: no constant)."""
    out = gen().matvec(gen().M, s)
    return out if k is None else [(x + c) % P for x, c in zip(out, k)]


def r_full_round(s, nxt):
    """12 S-boxes, MDS, round `nxt`'s constants."""
    return r_mds(r_sbox12(s), gen().RC[nxt])


def r_partial_round(s, nxt):
    """the plain partial round: S-box on lane 0, MDS, round `nxt`'s constants."""
    return r_mds([pow(s[0], 7, P)] + list(s[1:]), gen().RC[nxt])


def r_capz_round0(s):
    """round 0 with its constants, then round 1's constants."""
    return r_full_round([(x + c) % P for x, c in zip(s, gen().RC[0])], 1)


def r_init_sparse(s):
    _, init_rows, init_k, _, _ = derived()
    return [(x + k) % P for x, k in zip(gen().matvec(init_rows, s), init_k)]


def r_partial_group(s, t0):
    """partial rounds 4 + t0 .. of one group in the sparse form, round by round
    (the device defers lanes 1..11 over the group: the same map)."""
    A, _, _, kscalar, c26 = derived()
    s = list(s)
    for r in range(4 + t0, 4 + min(t0 + 4, 22)):
        ahat, b = A[r]
        x0 = pow(s[0], 7, P)
        k0 = kscalar[r + 1] if r < 25 else c26[0]
        n0 = (25 * x0 + sum(a * x for a, x in zip(ahat, s[1:])) + k0) % P
        s = [n0] + [(s[i] + b[i - 1] * x0 + (c26[i] if r == 25 else 0)) % P for i in range(1, 12)]
    return s


def r_rounds_from1(s):
    """rounds 1..29 of the plain permutation on the state entering round 1
    (round 1's constants already added)."""
    g = gen()
    s = list(s)
    for r in range(1, 30):
        if r > 1:
            s = [(x + c) % P for x, c in zip(s, g.RC[r])]
        if r < 4 or r >= 26:
            s = r_sbox12(s)
        else:
            s[0] = pow(s[0], 7, P)
        s = r_mds(s)
    return s


def r_composed(s):
    """The piece references in the order pf::permute_nc / pf::rounds<0> applies them."""
    s = [(x + c) % P for x, c in zip(s, gen().RC[0])]
    for nxt in (1, 2, 3):
        s = r_full_round(s, nxt)        # sbox12, mds_block<R + 1>
    s = r_init_sparse(r_sbox12(s))      # round 3: sbox12, mds_init_sparse
    for t0 in range(0, 22, 4):
        s = r_partial_group(s, t0)      # partial_group<T0, 4>, <20, 2>
    for nxt in (27, 28, 29):
        s = r_full_round(s, nxt)
    return r_mds(r_sbox12(s))           # round 29: mds_block<-1>


# ---- state sets ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def state_set(contract):
    """[n][12] u64 and the number of leading edge states.  contract "u64": any
    lanes; "capz": lanes 8..11 zero (edge lanes at positions 0..7 only)."""
    free = 12 if contract == "u64" else 8
    rng = np.random.default_rng(0x905E1D + free)
    rows = [np.full(12, e, np.uint64) for e in EDGE_VALUES]
    for e in EDGES:
        for j in range(free):
            r = rng.integers(0, 1 << 64, 12, dtype=np.uint64)
            r[j] = e
            rows.append(r)
    for j in range(free):
        r = np.full(12, M64, np.uint64)
        r[j] = rng.integers(0, 1 << 64, dtype=np.uint64)
        rows.append(r)
    nedge = len(rows)
    s = np.concatenate([np.stack(rows), rng.integers(0, 1 << 64, (NUNIFORM, 12), dtype=np.uint64)])
    if free < 12:
        s[:, free:] = 0
    s.setflags(write=False)
    return s, nedge


def ints(a):
    return [[int(x) for x in row] for row in np.asarray(a).tolist()]


def canon_rows(a):
    return [[x % P for x in row] for row in ints(a)]


@functools.lru_cache(maxsize=None)
def permuted(contract):
    """permute_plain of every state of the set, computed once."""
    return [gen().permute_plain(s) for s in canon_rows(state_set(contract)[0])]


INV7 = pow(7, -1, P - 1)


def carry_targets(coefs, k):
    """One MDS input vector per output row r whose reduce_row takes the carry:
    every used lane 0xFFFFFFFF00000000 (low halves 0: al = lo32(k[r])) except
    one lane of odd coefficient whose high half h makes lo32(ah) = 2^32 - 1,
    ah = sum_j coefs[r][j] hi_j + hi32(k[r]).  All values canonical."""
    out = []
    for r in range(12):
        used = [j for j in range(12) if coefs[r][j]]
        j0 = next(j for j in used if coefs[r][j] & 1)
        c, S = coefs[r][j0], sum(coefs[r])
        h = (M32 - (k[r] >> 32) + (S - c)) * pow(c, -1, 1 << 32) & M32
        y = [(M32 << 32) if j in used else 0 for j in range(12)]
        y[j0] = h << 32 if h < M32 else M32 << 32
        out.append(y)
    return out


def root7(y):
    return pow(y, INV7, P)


# ---- the MDS-type pieces: exact al, ah and reduce_row's steps -----------------

def halves(s):
    return s & U(M32), s >> U(32)


def dense_rows(s, k, coefs=None):
    """al, ah of the dense rows: sum_j coef[r][j] * half_j + half of k[r]
    (< 2^42: exact in u64)."""
    Mt = np.array(gen().M if coefs is None else coefs, dtype=np.uint64).T
    k = np.array(k, dtype=np.uint64)
    lo, hi = halves(s)
    return lo @ Mt + (k & U(M32)), hi @ Mt + (k >> U(32))


def raw_sbox(x):
    """pf::sbox as the gfn::mul step model has it (raw words)."""
    x2 = m_mul(x, x)[0]
    return m_mul(m_mul(x2, x)[0], m_mul(x2, x2)[0])[0]


def raw_add_c(a, c):
    """pf::add_c: a + c, + eps on a wrap."""
    s = a + c
    return s + (s < c).astype(np.uint64) * U(M32)


def limbs22(s):
    return np.stack([s & U(0x3FFFFF), (s >> U(22)) & U(0x3FFFFF), s >> U(44)], axis=-1)


def init_sparse_rows(s):
    """mds_init_sparse: row 0 the dense row with INIT_K[0]; rows 1..11 the
    22-bit limbs of all lanes times the halves of init_rows[i][j] 2^(22 k)."""
    g = gen()
    _, init_rows, init_k, _, _ = derived()
    al, ah = dense_rows(s, [init_k[0]] + [0] * 11)
    L = limbs22(s).reshape(s.shape[0], 36)
    cl = np.zeros((36, 12), np.uint64)
    ch = np.zeros((36, 12), np.uint64)
    for i in range(1, 12):
        for j in range(12):
            for kk, (l, h) in enumerate(g.limbs_consts(init_rows[i][j])):
                cl[3 * j + kk, i], ch[3 * j + kk, i] = l, h
    ik = np.array(init_k, dtype=np.uint64)
    al[:, 1:] = (L @ cl + (ik & U(M32)))[:, 1:]
    ah[:, 1:] = (L @ ch + (ik >> U(32)))[:, 1:]
    return al, ah


# piece name -> (form, param, contract, MDS input of a state (raw u64 array),
# (al, ah) of the MDS input, residue reference of a state, the constants k and
# coefficient rows of the carry construction or None, inverse of the input map
# for constructed MDS inputs)
def _rc(r):
    return gen().RC[r]


def _capz_coefs():
    return [[gen().M[r][j] if j < 8 else 0 for j in range(12)] for r in range(12)]


def piece(name):
    kind, _, par = name.partition(":")
    p = int(par) if par else 0
    ident = lambda s: s  # noqa: E731
    if kind == "mds_block":
        k = _rc(p) if p else [0] * 12
        return dict(form=N.PFORM_MDS_BLOCK, param=p, contract="u64", pre=ident, k=k,
                    ref=lambda s: r_mds(s, k if p else None), unpre=ident if p else None)
    if kind == "mds_k":
        return dict(form=N.PFORM_MDS_K, param=p, contract="u64", pre=ident, k=_rc(p),
                    ref=lambda s: r_mds(s, _rc(p)), unpre=ident)
    if kind in ("mds_mads", "coop_mds", "row_mds"):
        form = {"mds_mads": N.PFORM_MDS_MADS, "coop_mds": N.PFORM_COOP_MDS, "row_mds": N.PFORM_ROW_MDS}[kind]
        return dict(form=form, param=0, contract="u64", pre=ident, k=[0] * 12, ref=r_mds, unpre=None)
    if kind == "full_round_dyn":
        return dict(form=N.PFORM_FULL_ROUND_DYN, param=p, contract="u64", pre=raw_sbox, k=_rc(p),
                    ref=lambda s: r_full_round(s, p), unpre=lambda y: [root7(v) for v in y])
    if kind == "partial_dyn":
        def pre(s):
            s = s.copy()
            s[:, 0] = raw_sbox(s[:, 0])
            return s
        return dict(form=N.PFORM_PARTIAL_DYN, param=p, contract="u64", pre=pre, k=_rc(p),
                    ref=lambda s: r_partial_round(s, p), unpre=lambda y: [root7(y[0])] + y[1:])
    if kind == "capz_round0":
        def pre(s):
            y = raw_sbox(raw_add_c(s, np.array(_rc(0), dtype=np.uint64)))
            y[:, 8:] = 0
            return y
        return dict(form=N.PFORM_CAPZ_ROUND0, param=0, contract="capz", pre=pre, k=capz_k(), coefs=_capz_coefs(),
                    ref=r_capz_round0,
                    unpre=lambda y: [(root7(v) - c) % P if j < 8 else 0 for j, (v, c) in enumerate(zip(y, _rc(0)))])
    assert kind == "mds_init_sparse", name
    return dict(form=N.PFORM_MDS_INIT_SPARSE, param=0, contract="u64", pre=ident, rows=init_sparse_rows,
                k=[derived()[2][0]] + [0] * 11, only_rows=[0], ref=r_init_sparse, unpre=ident)


MDS_PIECES = (["mds_block", "mds_block:27", "mds_mads", "coop_mds", "row_mds", "capz_round0", "mds_init_sparse"] +
              [f"mds_k:{r}" for r in (1, 2, 3, 27, 28, 29)] +          # the quotient's Poseidon gate
              [f"full_round_dyn:{r}" for r in (1, 2, 3, 4, 27, 28, 29)] +  # the witness's rolled full rounds
              [f"partial_dyn:{r}" for r in range(5, 27)])              # ... and its rolled partial rounds


@functools.lru_cache(maxsize=None)
def piece_states(name):
    """The contract's state set, then the piece's constructed carry states."""
    pc = piece(name)
    s = state_set(pc["contract"])[0]
    if pc["unpre"] is None:
        return s
    rows = pc.get("only_rows", range(12))
    ys = carry_targets(pc.get("coefs", gen().M), pc["k"])
    extra = np.array([pc["unpre"](ys[r]) for r in rows], dtype=np.uint64)
    s = np.concatenate([s, extra])
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def piece_model(name):
    """(raw words, carry paths) of the piece on its states, from the exact al, ah."""
    pc = piece(name)
    with np.errstate(over="ignore"):
        y = pc["pre"](np.array(piece_states(name)))
        al, ah = pc["rows"](y) if "rows" in pc else dense_rows(y, pc["k"], pc.get("coefs"))
        assert int(al.max()) < 1 << 60 and int(ah.max()) < 1 << 60
        return m_reduce_row(al, ah)


@pytest.mark.parametrize("name", MDS_PIECES)
def test_state_set_takes_both_carries(name):
    """Every output lane's reduce_row takes its carry and its no-carry path
    somewhere in the piece's state set, and never a step documented as
    impossible."""
    _, path = piece_model(name)
    assert not (path & U(0b110)).any(), f"{name}: reduce_row wraps"
    for lane in range(12):
        assert set(np.unique(path[:, lane]).tolist()) == {0, 1}, f"{name}: lane {lane} misses a carry value"


@pytest.mark.parametrize("name", ["mds_block", "mds_block:27", "capz_round0", "mds_init_sparse", "mds_k:2",
                                  "full_round_dyn:4", "partial_dyn:5", "partial_dyn:26"])
def test_piece_models_agree_with_integers(name):
    """The restated steps give the reference's residue on the whole state set."""
    raw, _ = piece_model(name)
    ref = piece(name)["ref"]
    assert canon_rows(raw) == [ref(s) for s in canon_rows(piece_states(name))]


def test_piece_references_compose_to_the_plain_permutation():
    for contract in ("u64", "capz"):
        s = canon_rows(state_set(contract)[0])
        assert [r_composed(x) for x in s] == permuted(contract)
    # the capz round and the rounds<1> tail restate the same permutation
    s = canon_rows(state_set("capz")[0])
    assert [r_rounds_from1(r_capz_round0(x)) for x in s[:64] + s[-64:]] == permuted("capz")[:64] + permuted("capz")[-64:]


def test_state_sets_hold_what_they_claim():
    for contract, free in (("u64", 12), ("capz", 8)):
        s, nedge = state_set(contract)
        assert nedge == len(EDGE_VALUES) + len(EDGES) * free + free and len(s) == nedge + NUNIFORM
        assert set(EDGES) <= set(EDGE_VALUES) and {(h << 32) | l for h in HALVES for l in HALVES} <= set(EDGE_VALUES)
        assert (s[:len(EDGE_VALUES), :free] == np.array(EDGE_VALUES, np.uint64)[:, None]).all()
        assert (s[:, free:] == 0).all()
    assert len(state_set("u64")[0]) < (1 << 10) + 500


# ---- GPU ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def check_residues(out, ref, lanes, what):
    got = ints(out)
    assert len(got) == len(ref)
    assert all(0 <= w <= M64 for row in got for w in row)
    bad = [(i, j) for i, (g, r) in enumerate(zip(got, ref)) for j in lanes if g[j] % P != r[j]]
    assert not bad, f"{what}: {len(bad)} wrong residues, first at (state, lane) {bad[:4]}"


def row_layout(nedge, n):
    """Indices into a state set: each edge state at each of the four row
    positions of a wave in turn, its three neighbours uniform states."""
    idx, u = [], 0
    for e in range(nedge):
        for q in range(4):
            wave = [nedge + (u + i) % (n - nedge) for i in range(4)]
            wave[q] = e
            u += 3
            idx += wave
    return np.array(idx)


@gpu
@pytest.mark.parametrize("name", MDS_PIECES)
def test_mds_piece(ctx, name):
    """Residue against the integer reference, raw word against the documented
    steps, on a state set that takes both carries of every lane."""
    test_state_set_takes_both_carries(name)
    pc = piece(name)
    s = piece_states(name)
    out = N.debug_poseidon_op(ctx, pc["form"], s, param=pc["param"])
    check_residues(out, [pc["ref"](x) for x in canon_rows(s)], range(12), name)
    assert (out == piece_model(name)[0]).all(), f"{name}: raw result differs from the documented steps"


@gpu
@pytest.mark.parametrize("t0", [0, 4, 8, 12, 16, 20])
def test_partial_group(ctx, t0):
    """pf::partial_group<t0, 4> (<20, 2> folds KLAST): residues."""
    s = state_set("u64")[0]
    out = N.debug_poseidon_op(ctx, N.PFORM_PARTIAL_GROUP, s, param=t0)
    check_residues(out, [r_partial_group(x, t0) for x in canon_rows(s)], range(12), f"partial_group<{t0}>")


@gpu
def test_permute_nc(ctx):
    """pf::permute_nc on any u64 state (the carried-over sponge state)."""
    s = state_set("u64")[0]
    check_residues(N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, s), permuted("u64"), range(12), "permute_nc")


@gpu
def test_permute_nc_capz(ctx):
    """pf::permute_nc_capz<0xF> (Merkle and verifier nodes): lanes 0..3, which
    permute_nc must give too on the same states."""
    s = state_set("capz")[0]
    out = N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_CAPZ, s)
    check_residues(out, permuted("capz"), range(4), "permute_nc_capz<0xF>")
    full = N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, s)
    check_residues(full, permuted("capz"), range(12), "permute_nc on capz states")
    assert (out[:, :4] % U(P) == full[:, :4] % U(P)).all()


@gpu
def test_pow_tail_lane7(ctx):
    """pf::rounds<1, 0x80> (PoW): lane 7, on edge states entering round 1 and
    on the device's own round-0 output, where it must continue to permute_nc's
    lane 7."""
    s = state_set("u64")[0]
    out = N.debug_poseidon_op(ctx, N.PFORM_ROUNDS1_L7, s)
    check_residues(out, [r_rounds_from1(x) for x in canon_rows(s)], [7], "rounds<1, 0x80>")
    x0 = np.array([[(v + c) % P for v, c in zip(row, gen().RC[0])] for row in canon_rows(s)], dtype=np.uint64)
    r1 = N.debug_poseidon_op(ctx, N.PFORM_FULL_ROUND_DYN, x0, param=1)  # raw state entering round 1
    tail = N.debug_poseidon_op(ctx, N.PFORM_ROUNDS1_L7, r1)
    full = N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, s)
    check_residues(tail, permuted("u64"), [7], "rounds<1, 0x80> after round 0")
    assert (tail[:, 7] % U(P) == full[:, 7] % U(P)).all()


@gpu
@pytest.mark.parametrize("form", ["coop", "row"])
def test_cooperative_permute(ctx, form):
    """pc::permute (one state per wave) and pc::permute_row (four different
    states per wave, the edge state at each row position in turn): residues,
    and permute_nc's residues on the same states."""
    s, nedge = state_set("u64")
    op = N.PFORM_COOP_PERMUTE if form == "coop" else N.PFORM_ROW_PERMUTE
    idx = row_layout(nedge, len(s)) if form == "row" else np.arange(len(s))
    out = N.debug_poseidon_op(ctx, op, s[idx])
    ref = permuted("u64")
    check_residues(out, [ref[i] for i in idx], range(12), f"pc::permute ({form})")
    full = N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, s)
    assert (out % U(P) == full[idx] % U(P)).all()


@gpu
def test_wave_and_row_forms_agree_raw(ctx):
    """The same chain on the same values: pc::permute and pc::permute_row,
    pc::wave_mds_row and pc::row_mds give the same raw words, with each edge
    state at each row position among uniform neighbours."""
    s, nedge = state_set("u64")
    x = s[row_layout(nedge, len(s))]
    assert (N.debug_poseidon_op(ctx, N.PFORM_COOP_PERMUTE, x) == N.debug_poseidon_op(ctx, N.PFORM_ROW_PERMUTE, x)).all()
    mw, mr = N.debug_poseidon_op(ctx, N.PFORM_COOP_MDS, x), N.debug_poseidon_op(ctx, N.PFORM_ROW_MDS, x)
    assert (mw == mr).all()
    with np.errstate(over="ignore"):
        assert (mr == m_reduce_row(*dense_rows(x, [0] * 12))[0]).all(), "row_mds: raw result differs from the steps"
    check_residues(mr, [r_mds(v) for v in canon_rows(x)], range(12), "row_mds in the row layout")


@gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 17])
def test_rows_and_waves_past_the_end(ctx, n):
    """State counts that leave rows of the last wave, and waves of the last
    block, without a state: they exit whole and the others are unaffected."""
    s, nedge = state_set("u64")
    idx = row_layout(nedge, len(s))[:n]
    x = s[idx]
    ref = permuted("u64")
    for op, what in ((N.PFORM_ROW_PERMUTE, "permute_row"), (N.PFORM_COOP_PERMUTE, "permute")):
        check_residues(N.debug_poseidon_op(ctx, op, x), [ref[i] for i in idx], range(12), f"pc::{what} x{n}")
    for op, what in ((N.PFORM_ROW_MDS, "row_mds"), (N.PFORM_COOP_MDS, "wave_mds_row")):
        check_residues(N.debug_poseidon_op(ctx, op, x), [r_mds(v) for v in canon_rows(x)], range(12), f"pc::{what} x{n}")


@gpu
def test_probe_rejects_bad_arguments(ctx):
    import qp_wormhole
    ok = np.zeros((2, 12), np.uint64)
    bad = [(N.PFORM_COUNT, 0), (N.PFORM_PERMUTE_NC, 1), (N.PFORM_MDS_BLOCK, 1), (N.PFORM_MDS_BLOCK, 26),
           (N.PFORM_MDS_K, 0), (N.PFORM_MDS_K, 30), (N.PFORM_FULL_ROUND_DYN, 0), (N.PFORM_FULL_ROUND_DYN, 30),
           (N.PFORM_PARTIAL_DYN, 30), (N.PFORM_PARTIAL_GROUP, 2), (N.PFORM_PARTIAL_GROUP, 24), (N.PFORM_ROW_MDS, 4)]
    for form, param in bad:
        with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
            N.debug_poseidon_op(ctx, form, ok, param=param)
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, None)
    for form in (N.PFORM_PERMUTE_CAPZ, N.PFORM_CAPZ_ROUND0):
        for lane in range(8, 12):
            x = ok.copy()
            x[1, lane] = 1
            with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
                N.debug_poseidon_op(ctx, form, x)
    assert lib_rc_null_out(ctx) == 1
    assert N.debug_poseidon_op(ctx, N.PFORM_PERMUTE_NC, np.zeros((0, 12), np.uint64)).shape == (0, 12)


def lib_rc_null_out(ctx):
    """the raw status of a call whose out pointer is null (QP_ERR_ARG = 1)"""
    s = np.zeros(12, np.uint64)
    return N.lib().qp_debug_poseidon_op(ctx.h, int(N.PFORM_PERMUTE_NC), 0, s.ctypes.data, 1, None)
