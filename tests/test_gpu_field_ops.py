"""Edge-value tests of the device field arithmetic, one function at a time.

The hot kernels do not use the readable gl:: functions: they run hand-written
carry chains and inline assembly on non-canonical values in [0, 2^64)
(field_nc.h gfn::, which holds the general products mul, mul_c and mulk<K> that
the PF_MUL* ops probe, and ntt16.h nt:: and poseidon_fast.h pf:: built on it).
Under uniform inputs a single wrap or borrow in those chains has probability
about 2^-32 and the double wraps about 2^-64, so the bit-exact whole-kernel
tests never take them.
Here the TEST-ONLY probe qp_debug_field_op (csrc/field_probe.hip) applies one
device function per lane to chosen operands and returns the raw u64:

  * the reference is Python integer arithmetic, never the C oracle;
  * the operands are the full cross product of an edge list with itself plus
    2^16 uniform pairs (restricted to the function's own contract);
  * a CPU-side coverage condition (also run without a GPU) restates the
    documented steps of the carry chains as numpy u64 arithmetic, records which
    carries and borrows every operand takes, and requires every combination a
    fixed-seed search finds reachable to be present in the operand set: an edit
    of the operand list cannot quietly drop the rare paths;
  * on the GPU the raw result must also equal that restatement, so the
    restatement describes the code whose paths it counts.
"""
import functools

import numpy as np
import pytest

from edge_values import EDGES, P
from qp_wormhole import _native as N

gpu = pytest.mark.gpu

M64 = (1 << 64) - 1
U = np.uint64
EPS = U(0xFFFFFFFF)
S32 = U(32)

HALVES = [0, 1, 2**31, 2**32 - 2, 2**32 - 1]
EDGE_VALUES = sorted(set(EDGES) | {(h << 32) | lo for h in HALVES for lo in HALVES})
# the bounded operands of pf::reduce_row (al, ah < 2^60; lt42 is the range of
# the dense MDS rows, lt60 the guaranteed domain that the sparse partial rounds
# use up to 2^58.2) and pf::sub_small (y < 2^40)
EDGES_42 = sorted({v for v in EDGE_VALUES if v < 2**42} |
                  {2**41, 2**42 - 2**32 - 1, 2**42 - 2**32, 2**42 - 2**32 + 1, 2**42 - 2, 2**42 - 1,
                   2**41 + 2**32 - 1, 2**33, 2**41 - 1})
EDGES_40 = sorted({v for v in EDGE_VALUES if v < 2**40} |
                  {2**39, 2**40 - 2**32 - 1, 2**40 - 2**32, 2**40 - 2, 2**40 - 1, 2**33})
HALVES_28 = [0, 1, 2**27, 2**28 - 2, 2**28 - 1]
EDGES_60 = sorted({v for v in EDGE_VALUES if v < 2**60} |
                  {(h << 32) | lo for h in HALVES_28 for lo in HALVES} |
                  {2**60 - 2**32 - 1, 2**60 - 2**32, 2**60 - 2**32 + 1, 2**60 - 2, 2**60 - 1,
                   2**59 - 1, 2**59, 2**59 + 1, 2**59 + 2**32 - 1, ((2**28 - 1) << 32) | 0xFFFFFFFF,
                   ((2**28 - 1) << 32) | 0xFFFFFFFE, (2**28 - 1) << 32})
NRAND = 1 << 16

DOMAINS = {"u64": (EDGE_VALUES, 1 << 64), "canon": ([v for v in EDGE_VALUES if v < P], P),
           "lt42": (EDGES_42, 1 << 42), "lt40": (EDGES_40, 1 << 40), "lt60": (EDGES_60, 1 << 60)}


def u64(v):
    return np.array(v, dtype=np.uint64)


def lo32(x):
    return x & EPS


def hi32(x):
    return x >> S32


def bit(c):
    return c.astype(np.uint64)


# ---- the documented steps, as numpy u64 arithmetic (wrapping) ---------------
# every model returns (raw result, path): path packs the carries / borrows the
# operand takes, one bit each; NEVER[name] masks the bits the code documents as
# "cannot happen" (it has no instruction for them)

def m_add(a, b):
    """nt::add_mad / nt::add4 / gfn::add: s = a + b; on a wrap + eps; wrapped
    again (both inputs in [p, 2^64)) + eps, which cannot wrap."""
    s = a + b
    c1 = bit(s < a)
    s2 = s + c1 * EPS
    c2 = bit(s2 < s)
    s3 = s2 + c2 * EPS
    c3 = bit(s3 < s2)
    return s3, c1 | c2 << U(1) | c3 << U(2)


def m_sub(a, b):
    """gfn::sub / nt::sub4: d = a - b; on a borrow - eps; on a second borrow
    (b > a + p) - eps again, which cannot borrow."""
    d = a - b
    b1 = bit(a < b)
    d2 = d - b1 * EPS
    b2 = bit(d < b1 * EPS)
    d3 = d2 - b2 * EPS
    b3 = bit(d2 < b2 * EPS)
    return d3, b1 | b2 << U(1) | b3 << U(2)


def m_nt_reduce(lo, hi):
    """nt::reduce: lo - hh (borrow: - eps, cannot borrow again) + hl eps
    (carry: + eps, cannot carry again)."""
    hh, hl = hi32(hi), lo32(hi)
    t0 = lo - hh
    bo = bit(lo < hh)
    t0b = t0 - bo * EPS
    bo2 = bit(t0 < bo * EPS)
    t1 = (hl << S32) - hl
    r = t0b + t1
    c = bit(r < t1)
    r2 = r + c * EPS
    c2 = bit(r2 < r)
    return r2, bo | bo2 << U(1) | c << U(2) | c2 << U(3)


def m_gfn_reduce(lo, hi):
    """gfn::reduce, on 32-bit halves as the code has it."""
    hl, hh = lo32(hi), hi32(hi)
    l0, l1 = lo32(lo), hi32(lo)
    bo = bit(l0 < hh)
    l0 = lo32(l0 - hh)
    bo2 = bit(l1 < bo)
    l1 = lo32(l1 - bo)
    c = bit(l0 + bo2 > EPS)
    l0 = lo32(l0 + bo2)
    l1 = lo32(l1 - bo2 + c)
    bt = bit(hl != 0)
    t0, t1 = lo32(U(0) - hl), hl - bt
    ca = bit(l0 + t0 > EPS)
    l0 = lo32(l0 + t0)
    cb = bit(l1 + t1 + ca > EPS)
    l1 = lo32(l1 + t1 + ca)
    e = lo32(U(0) - cb)
    cc = bit(l0 + e > EPS)
    l0 = lo32(l0 + e)
    cd = bit(l1 + cc > EPS)  # documented: cannot carry out
    l1 = lo32(l1 + cc)
    return l1 << S32 | l0, bo2 | c << U(1) | cb << U(2) | cc << U(3) | cd << U(4)


def m_reduce_row(al, ah):
    """pf::reduce_row / reduce_row_c for al, ah < 2^60: t = al + eps hi32(ah)
    (< 2^61: cannot wrap); t.hi += lo32(ah) with carry c (worth 2^64 = eps);
    + c eps (on a carry the new t.hi < 2^29: cannot wrap)."""
    t = al + hi32(ah) * EPS
    ct = bit(t < al)
    t1 = hi32(t) + lo32(ah)
    c = hi32(t1)
    tt = lo32(t1) << S32 | lo32(t)
    r = tt + c * EPS
    c3 = bit(r < tt)
    return r, c | ct << U(1) | c3 << U(2)


def m_mul(a, b):
    """gfn::mul: U = a1 b0 + T with carry cu; W = a1 b1 + (U.hi | cu << 32);
    t = X + eps w2 (carry c1: + eps, cannot wrap); r = t - w3 (borrow: - eps,
    cannot borrow)."""
    a0, a1, b0, b1 = lo32(a), hi32(a), lo32(b), hi32(b)
    L = a0 * b0
    T = a0 * b1 + hi32(L)
    Uu = a1 * b0 + T
    cu = bit(Uu < T)
    W = a1 * b1 + (cu << S32 | hi32(Uu))
    X = lo32(Uu) << S32 | lo32(L)
    t = X + lo32(W) * EPS
    c1 = bit(t < X)
    t2 = t + c1 * EPS
    c2 = bit(t2 < t)
    w3 = hi32(W)
    r = t2 - w3
    c3 = bit(t2 < w3)
    r2 = r - c3 * EPS
    c4 = bit(r < c3 * EPS)
    return r2, cu | c1 << U(1) | c2 << U(2) | c3 << U(3) | c4 << U(4)


def m_mul_pow2(x, E):
    """nt::mul_pow2<E>: the three shift regimes, E >= 96 as neg() of E - 96
    (bits 5, 6: the canon() subtraction and the zero case of neg)."""
    if E >= 96:
        r, path = m_mul_pow2(x, E - 96)
        c = bit(r >= U(P))
        r = r - c * U(P)
        z = bit(r == 0)
        return (U(P) - r) * (U(1) - z), path | c << U(5) | z << U(6)
    if E == 0:
        return x.copy(), np.zeros_like(x)
    if E < 64:
        lo, hi = x << U(E), x >> U(64 - E)
    if E < 32:
        return m_nt_reduce(lo, hi)
    if E < 64:
        # lo + h0 eps (carry: + eps, stays below 2^64) - h1 (borrow: - eps, cannot borrow again)
        h0, h1 = lo32(hi), hi32(hi)
        t = lo + h0 * EPS
        c = bit(t < lo)
        t2 = t + c * EPS
        c2 = bit(t2 < t)
        r = t2 - h1
        b = bit(t2 < h1)
        r2 = r - b * EPS
        b2 = bit(r < b * EPS)
        return r2, c | c2 << U(1) | b << U(2) | b2 << U(3)
    # (u0 << 32) - S, S = u0 + u1 + v (borrow: - eps, cannot borrow again)
    F = U(E - 64)
    u, v = lo32(x) << F, hi32(x) << F
    S = v + lo32(u) + hi32(u)
    A = lo32(u) << S32
    r = A - S
    b = bit(A < S)
    r2 = r - b * EPS
    b2 = bit(r < b * EPS)
    return r2, b | b2 << U(1)


def m_acc3(a, b, K):
    """gfn::Acc3 over groups of K: mac(a[k], b[k]) for each, add_shifted(a[0],
    K % 64), value().  Returns (raw values, the set of mac paths): bit 0 the
    carry cl out of a0 b0 + lo, bit 1 the carry cu of the middle column, bit 2
    the carry into top, bit 3 an overflow of W (documented: cannot happen)."""
    a, b = a.reshape(-1, K), b.reshape(-1, K)
    lo, hi, top = (np.zeros(a.shape[0], np.uint64) for _ in range(3))
    paths = set()
    for k in range(K):
        a0, a1, b0, b1 = lo32(a[:, k]), hi32(a[:, k]), lo32(b[:, k]), hi32(b[:, k])
        L = a0 * b0 + lo
        cl = bit(L < lo)
        T = a0 * b1 + hi32(L)
        Uu = a1 * b0 + T
        cu = bit(Uu < T)
        W = a1 * b1 + (cu << S32 | hi32(Uu))
        cw = bit(W < a1 * b1)
        lo = lo32(Uu) << S32 | lo32(L)
        s = hi + W
        ct = bit(s < hi)
        s2 = s + cl
        ct |= bit(s2 < s)
        hi = s2
        top = top + ct
        paths |= set(np.unique(cl | cu << U(1) | ct << U(2) | cw << U(3)).tolist())
    e = K % 64
    x = a[:, 0]
    xl, xh = x << U(e), (x >> U(64 - e) if e else np.zeros_like(x))
    l2 = lo + xl
    c = bit(l2 < lo)
    h2 = hi + xh
    ch = bit(h2 < hi)
    h3 = h2 + c
    ch |= bit(h3 < h2)
    top = top + ch
    assert (top < U(1 << 32)).all()
    r, _ = m_gfn_reduce(l2, h3)
    return m_sub(r, top << S32)[0], paths


NEVER = {"reduce_row": 0b110, "add": 0b100, "sub": 0b100, "nt_reduce": 0b1010, "gfn_reduce": 0b10000, "mul": 0b10100, "acc3_mac": 0b1000}


def never_pow2(E):
    E %= 96
    return 0 if E == 0 else 0b1010 if E < 64 else 0b10


# ---- operand sets ------------------------------------------------------------

def rand_in(rng, n, bound):
    return rng.integers(0, bound, size=n, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def pair_set(dom_a, dom_b):
    """Full cross product of the two domains' edge lists, then 2^16 uniform pairs."""
    (ea, ba), (eb, bb) = DOMAINS[dom_a], DOMAINS[dom_b]
    rng = np.random.default_rng(0xF1E1D)
    a = np.concatenate([np.repeat(u64(ea), len(eb)), rand_in(rng, NRAND, ba)])
    b = np.concatenate([np.tile(u64(eb), len(ea)), rand_in(rng, NRAND, bb)])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def value_set():
    rng = np.random.default_rng(0xF1E1E)
    a = np.concatenate([u64(EDGE_VALUES), rand_in(rng, NRAND, 1 << 64)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def group_set(K, every_position):
    """K-wide operands: each edge pair at position j of a group whose other
    K - 1 pairs are uniform (every j in turn, or j cycling through the
    positions pair by pair), then uniform groups and one all-maximal group."""
    ea, eb = pair_set("u64", "u64")
    npairs = len(EDGE_VALUES) ** 2
    ea, eb = ea[:npairs], eb[:npairs]
    rng = np.random.default_rng(0xF1E1F + K)
    positions = range(K) if every_position else [None]
    blocks_a, blocks_b = [], []
    for j in positions:
        ga, gb = rand_in(rng, npairs * K, 1 << 64).reshape(-1, K), rand_in(rng, npairs * K, 1 << 64).reshape(-1, K)
        col = np.full(npairs, j) if j is not None else np.arange(npairs) % K
        ga[np.arange(npairs), col] = ea
        gb[np.arange(npairs), col] = eb
        blocks_a.append(ga)
        blocks_b.append(gb)
    nr = -(-NRAND // K)
    blocks_a += [rand_in(rng, nr * K, 1 << 64).reshape(-1, K), np.full((1, K), M64, np.uint64)]
    blocks_b += [rand_in(rng, nr * K, 1 << 64).reshape(-1, K), np.full((1, K), M64, np.uint64)]
    a, b = np.concatenate(blocks_a).ravel(), np.concatenate(blocks_b).ravel()
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def structured(rng, n):
    """Search candidates: halves from the edge halves or uniform; edge values
    +- a small step; values within 2^33 of 0, p and 2^64; uniform."""
    parts = []
    q = n // 4
    hv = u64(HALVES + [2, 2**31 - 1, 2**31 + 1, 2**32 - 3])
    for _ in range(1):
        h = np.where(rng.random(q) < 0.7, hv[rng.integers(0, len(hv), q)], rand_in(rng, q, 1 << 32))
        lo = np.where(rng.random(q) < 0.7, hv[rng.integers(0, len(hv), q)], rand_in(rng, q, 1 << 32))
        parts.append(h << S32 | lo)
    ev = u64(EDGE_VALUES)
    parts.append(ev[rng.integers(0, len(ev), q)] + rng.integers(-4, 5, q).astype(np.int64).astype(np.uint64))
    base = u64([0, P, 0])[rng.integers(0, 3, q)]  # 0 - d wraps to just below 2^64
    d = rand_in(rng, q, 1 << 33)
    parts.append(np.where(rng.random(q) < 0.5, base + d, base - d))
    parts.append(rand_in(rng, n - 3 * q, 1 << 64))
    out = np.concatenate(parts)
    rng.shuffle(out)
    return out


NSEARCH = 1 << 20


@functools.lru_cache(maxsize=None)
def search_pairs(dom_a, dom_b):
    """The search space: the edge cross product plus 2^20 structured candidates
    (an eighth of them correlated: b = a + an edge value)."""
    rng = np.random.default_rng(0x5EA4C)
    a, b = structured(rng, NSEARCH), structured(rng, NSEARCH)
    k = NSEARCH // 8
    ev = u64(EDGE_VALUES)
    b[:k] = a[:k] + ev[rng.integers(0, len(ev), k)]
    (ea, ba), (eb, bb) = DOMAINS[dom_a], DOMAINS[dom_b]
    if ba < 1 << 64:
        a = a % U(ba)
    if bb < 1 << 64:
        b = b % U(bb)
    a = np.concatenate([np.repeat(u64(ea), len(eb)), a])
    b = np.concatenate([np.tile(u64(eb), len(ea)), b])
    return a, b


def paths_of(path):
    return sorted(int(p) for p in np.unique(path))


# ---- the committed lists of reachable combinations ---------------------------
# (search_pairs / search over value candidates, seed fixed above;
# test_reachable_lists_are_current recomputes them)
REACHABLE = {
    "add": [0, 1, 3],
    "sub": [0, 1, 3],
    "nt_reduce": [0, 1, 4, 5],
    "gfn_reduce": [0, 1, 3, 4, 5, 12, 13, 15],
    "mul": [0, 1, 2, 3, 8],  # a borrow of t - w3 (8) only without the carries cu and c1
    "acc3_mac": [0, 1, 2, 3, 4, 5, 6, 7],
    "reduce_row": [0, 1],
}
# mul_pow2<E>, the same for every E of a shift regime
REACHABLE_POW2 = {E: [0] if E == 0 else [0, 4] if E < 32 else [0, 1, 4] if E < 64 else [0, 1] if E < 96 else
                  [0, 32, 64, 96] if E == 96 else [0, 4, 32, 64, 96] if E < 128 else
                  [0, 1, 4, 32, 64, 96] if E < 160 else [0, 1, 64] for E in range(0, 192, 6)}

MODELLED = {
    # name: (model, operand domains)
    "add": (m_add, ("u64", "u64")),
    "sub": (m_sub, ("u64", "u64")),
    "nt_reduce": (m_nt_reduce, ("u64", "u64")),
    "gfn_reduce": (m_gfn_reduce, ("u64", "u64")),
    "mul": (m_mul, ("u64", "u64")),
    "reduce_row": (m_reduce_row, ("lt60", "lt60")),
}
POW2_E = list(range(0, 192, 6))
ACC3_K = [1, 2, 16, 123]


def acc3_operands(K):
    return group_set(K, K <= 16)


@functools.lru_cache(maxsize=None)
def operand_paths(name):
    """The combinations the operand set of `name` takes (4-wide forms: the
    operands of every position)."""
    with np.errstate(over="ignore"):
        if name == "acc3_mac":
            return sorted(set().union(*(m_acc3(*acc3_operands(K), K)[1] for K in ACC3_K)))
        if name.startswith("pow2_"):
            return paths_of(m_mul_pow2(value_set(), int(name[5:]))[1])
        model, doms = MODELLED[name]
        got = set(paths_of(model(*pair_set(*doms))[1]))
        if name in ("add", "sub"):
            got &= set(paths_of(model(*group_set(4, True))[1]))
        return sorted(got)


def reachable(name):
    return REACHABLE_POW2[int(name[5:])] if name.startswith("pow2_") else REACHABLE[name]


def never(name):
    return never_pow2(int(name[5:])) if name.startswith("pow2_") else NEVER[name]


def check_coverage(name):
    """Every reachable combination is in the operand set at least once, and no
    operand takes a step the code has no instruction for."""
    got, want = operand_paths(name), reachable(name)
    assert want, name
    missing = sorted(set(want) - set(got))
    assert not missing, f"{name}: operand set lost the carry/borrow combinations {missing}"
    assert not [p for p in got if p & never(name)], f"{name}: a documented 'cannot happen' step is reachable"


COVERED = list(MODELLED) + ["acc3_mac"] + [f"pow2_{E}" for E in POW2_E]


@pytest.mark.parametrize("name", COVERED)
def test_operand_set_covers_reachable_paths(name):
    check_coverage(name)


def search_paths(name):
    with np.errstate(over="ignore"):
        if name == "acc3_mac":
            rng = np.random.default_rng(0x5EA4D)
            found = set()
            for K in ACC3_K:
                n = NSEARCH // K * K
                found |= m_acc3(structured(rng, NSEARCH)[:n], structured(rng, NSEARCH)[:n], K)[1]
                found |= m_acc3(*acc3_operands(K), K)[1]
            return sorted(found)
        if name.startswith("pow2_"):
            x = np.concatenate([u64(EDGE_VALUES), search_pairs("u64", "u64")[0]])
            return paths_of(m_mul_pow2(x, int(name[5:]))[1])
        model, doms = MODELLED[name]
        return paths_of(model(*search_pairs(*doms))[1])


@pytest.mark.parametrize("name", COVERED)
def test_reachable_lists_are_current(name):
    """The committed lists are what the fixed-seed search over the edge cross
    product plus 2^20 structured candidates finds, and none of them takes a
    step documented as impossible (that would be a bug in the header)."""
    found = search_paths(name)
    assert found == reachable(name), (name, found)
    assert not [p for p in found if p & never(name)], (name, found)


def ints(a):
    return [int(x) for x in a.tolist()] if isinstance(a, np.ndarray) else a


def residues(a):
    return [x % P for x in ints(a)]


@pytest.mark.parametrize("name", COVERED)
def test_models_agree_with_integers(name):
    """The restated steps compute the right residue on the whole operand set."""
    with np.errstate(over="ignore"):
        if name == "acc3_mac":
            for K in ACC3_K:
                a, b = acc3_operands(K)
                assert residues(m_acc3(a, b, K)[0]) == ref_acc3(ints(a), ints(b), K)
            return
        if name.startswith("pow2_"):
            E = int(name[5:])
            assert residues(m_mul_pow2(value_set(), E)[0]) == [(x << E) % P for x in ints(value_set())]
            return
        model, doms = MODELLED[name]
        a, b = pair_set(*doms)
        ref = {"add": lambda x, y: (x + y) % P, "sub": lambda x, y: (x - y) % P, "mul": lambda x, y: x * y % P,
               "nt_reduce": lambda x, y: (x + (y << 64)) % P, "gfn_reduce": lambda x, y: (x + (y << 64)) % P,
               "reduce_row": lambda x, y: (x + (y << 32)) % P}[name]
        assert residues(model(a, b)[0]) == [ref(x, y) for x, y in zip(ints(a), ints(b))]


def ref_acc3(a, b, K):
    return [(sum(x * y for x, y in zip(a[g:g + K], b[g:g + K])) + (a[g] << (K % 64))) % P
            for g in range(0, len(a), K)]


# ---- GPU ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def check(out, ref, canonical=False, what=""):
    """Exact residue; a documented range where there is one."""
    got = ints(out)
    assert len(got) == len(ref)
    bad = [i for i, (g, r) in enumerate(zip(got, ref)) if g % P != r]
    assert not bad, f"{what}: {len(bad)} wrong residues, first at {bad[:4]}"
    assert all(0 <= g <= M64 for g in got)
    if canonical:
        assert all(g < P for g in got), f"{what}: result not canonical"


BINARY = {
    # name: (op, domains, reference, canonical out, model with the same raw result)
    "nt_add": (N.FOP_NT_ADD, ("u64", "u64"), lambda a, b: (a + b) % P, False, "add"),
    "gfn_add": (N.FOP_GFN_ADD, ("u64", "u64"), lambda a, b: (a + b) % P, False, "add"),
    "gfn_add_c": (N.FOP_GFN_ADD_C, ("u64", "canon"), lambda a, b: (a + b) % P, False, None),
    "pf_add_c": (N.FOP_PF_ADD_C, ("u64", "canon"), lambda a, b: (a + b) % P, False, None),
    "gl_add": (N.FOP_GL_ADD, ("canon", "canon"), lambda a, b: (a + b) % P, True, None),
    "nt_sub": (N.FOP_NT_SUB, ("u64", "u64"), lambda a, b: (a - b) % P, False, "sub"),
    "gl_sub": (N.FOP_GL_SUB, ("canon", "canon"), lambda a, b: (a - b) % P, True, None),
    "nt_reduce": (N.FOP_NT_REDUCE, ("u64", "u64"), lambda a, b: (a + (b << 64)) % P, False, "nt_reduce"),
    "gfn_reduce": (N.FOP_GFN_REDUCE, ("u64", "u64"), lambda a, b: (a + (b << 64)) % P, False, "gfn_reduce"),
    "gl_reduce128": (N.FOP_GL_REDUCE128, ("u64", "u64"), lambda a, b: (a + (b << 64)) % P, True, None),
    "pf_reduce_row": (N.FOP_PF_REDUCE_ROW, ("lt42", "lt42"), lambda a, b: (a + (b << 32)) % P, False, None),
    "pf_reduce_row_c": (N.FOP_PF_REDUCE_ROW_C, ("lt42", "lt42"), lambda a, b: (a + (b << 32)) % P, False, None),
    "pf_reduce_row_60": (N.FOP_PF_REDUCE_ROW, ("lt60", "lt60"), lambda a, b: (a + (b << 32)) % P, False,
                         "reduce_row"),
    "pf_reduce_row_c_60": (N.FOP_PF_REDUCE_ROW_C, ("lt60", "lt60"), lambda a, b: (a + (b << 32)) % P, False,
                           "reduce_row"),
    "pf_sub_small": (N.FOP_PF_SUB_SMALL, ("u64", "lt40"), lambda a, b: (a - b) % P, False, None),
    "pf_mul": (N.FOP_PF_MUL, ("u64", "u64"), lambda a, b: a * b % P, False, "mul"),
    "pf_mul_c": (N.FOP_PF_MUL_C, ("u64", "u64"), lambda a, b: a * b % P, False, "mul"),
    "gl_mul": (N.FOP_GL_MUL, ("u64", "u64"), lambda a, b: a * b % P, True, None),
}


@gpu
@pytest.mark.parametrize("name", list(BINARY))
def test_binary_op(ctx, name):
    op, doms, ref, canonical, model = BINARY[name]
    if model:
        check_coverage(model)
    a, b = pair_set(*doms)
    out = N.debug_field_op(ctx, op, a, b)
    check(out, [ref(x, y) for x, y in zip(ints(a), ints(b))], canonical, name)
    if model:
        with np.errstate(over="ignore"):
            assert (out == MODELLED[model][0](a, b)[0]).all(), f"{name}: raw result differs from the documented steps"


@gpu
@pytest.mark.parametrize("name,op,model", [("nt_add4", N.FOP_NT_ADD4, "add"), ("nt_sub4", N.FOP_NT_SUB4, "sub")])
def test_four_wide(ctx, name, op, model):
    """add4 / sub4 with each edge pair at each of the four positions among
    uniform neighbours: a carry register crossed between the interleaved
    chains gives the neighbour's correction to the edge pair."""
    check_coverage(model)
    a, b = group_set(4, True)
    out = N.debug_field_op(ctx, op, a, b)
    sign = 1 if model == "add" else -1
    check(out, [(x + sign * y) % P for x, y in zip(ints(a), ints(b))], False, name)
    with np.errstate(over="ignore"):
        assert (out == MODELLED[model][0](a, b)[0]).all()
    assert (out == N.debug_field_op(ctx, N.FOP_NT_ADD if model == "add" else N.FOP_NT_SUB, a, b)).all()


@gpu
def test_products_agree_raw(ctx):
    """gfn::mul, gfn::mul_c and gfn::mulk<2|3> claim the same arithmetic: equal as
    raw u64, with each edge pair at each position of the K-wide forms."""
    check_coverage("mul")
    a, b = pair_set("u64", "u64")
    m = N.debug_field_op(ctx, N.FOP_PF_MUL, a, b)
    assert (m == N.debug_field_op(ctx, N.FOP_PF_MUL_C, a, b)).all()
    for K, op in ((2, N.FOP_PF_MULK2), (3, N.FOP_PF_MULK3)):
        ga, gb = group_set(K, True)
        out = N.debug_field_op(ctx, op, ga, gb)
        check(out, [x * y % P for x, y in zip(ints(ga), ints(gb))], False, f"mulk<{K}>")
        assert (out == N.debug_field_op(ctx, N.FOP_PF_MUL, ga, gb)).all(), K
        n = len(a) // K * K
        assert (N.debug_field_op(ctx, op, a[:n], b[:n]) == m[:n]).all(), K


@gpu
@pytest.mark.parametrize("name,op", [("pf_sbox", N.FOP_PF_SBOX), ("pf_sbox_c", N.FOP_PF_SBOX_C)])
def test_sbox(ctx, name, op):
    a = value_set()
    out = N.debug_field_op(ctx, op, a)
    check(out, [pow(x, 7, P) for x in ints(a)], False, name)
    assert (out == N.debug_field_op(ctx, N.FOP_PF_SBOX, a)).all()


@gpu
@pytest.mark.parametrize("E", POW2_E)
def test_mul_pow2(ctx, E):
    """Every shift the transforms instantiate (mul_w16<INV, J>, mul_w32<INV>)."""
    check_coverage(f"pow2_{E}")
    a = value_set()
    out = N.debug_field_op(ctx, N.FOP_NT_MUL_POW2, a, param=E)
    check(out, [(x << E) % P for x in ints(a)], False, f"mul_pow2<{E}>")
    with np.errstate(over="ignore"):
        assert (out == m_mul_pow2(a, E)[0]).all()


@gpu
@pytest.mark.parametrize("K", ACC3_K)
def test_acc3(ctx, K):
    check_coverage("acc3_mac")
    a, b = acc3_operands(K)
    out = N.debug_field_op(ctx, N.FOP_ACC3, a, b, param=K)
    check(out, ref_acc3(ints(a), ints(b), K), False, f"Acc3 x{K}")
    with np.errstate(over="ignore"):
        assert (out == m_acc3(a, b, K)[0]).all()


@gpu
def test_probe_rejects_bad_arguments(ctx):
    import qp_wormhole
    a = np.zeros(12, np.uint64)
    for op, param, n in ((N.FOP_COUNT, 0, 12), (N.FOP_NT_ADD, 1, 12), (N.FOP_NT_MUL_POW2, 7, 12),
                         (N.FOP_NT_MUL_POW2, 192, 12), (N.FOP_ACC3, 0, 12), (N.FOP_NT_ADD4, 0, 10),
                         (N.FOP_PF_MULK3, 0, 10), (N.FOP_ACC3, 5, 12)):
        with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
            N.debug_field_op(ctx, op, a[:n], a[:n], param=param)
