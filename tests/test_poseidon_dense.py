"""The small-integer grouped form of Poseidon's partial rounds that the hashing
permutation runs (tools/gen_poseidon_dense.py -> csrc/poseidon_dense_consts.h,
pf::dense_group in poseidon_fast.h):

  * the committed header is what the generator emits;
  * its tables, parsed from the header text, equal (MZ)^m and (MZ)^k M e_0
    computed here from M with numpy object matrices, and its constants equal
    the round constants pushed through those maps;
  * the grouped form evaluated from the parsed tables, between the plain full
    rounds, is the plain permutation;
  * with every 32-bit half at 2^32 - 1 every accumulator stays inside the
    domain reduce_row is tested on (test_gpu_field_ops.py "lt60") and
    reduce_row's own t = al + eps hi32(ah) stays below 2^64.

The numpy step model of pf::dense_group (exact al, ah of every row, then
m_reduce_row, S-boxes as gfn::mul chains) and the state set with both carry
values of every row live here too; tests/test_gpu_poseidon_dense.py compares
the device's raw words with them.
"""
import functools
import importlib.util
import math
import os
import random
import re

import numpy as np
import pytest

from edge_values import P
from test_gpu_field_ops import DOMAINS, m_reduce_row
from test_gpu_poseidon_forms import INV7, canon_rows, carry_targets, halves, raw_sbox, state_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "qp-zk-circuits-rm_amd", "csrc", "poseidon_dense_consts.h")
M32 = (1 << 32) - 1
U = np.uint64
PLAN = (3, 3, 3, 3, 3, 3, 2, 2)  # the shipped plan
STARTS = (0, 3, 6, 9, 12, 15, 18, 20)


@functools.lru_cache(maxsize=None)
def gen():
    spec = importlib.util.spec_from_file_location("gen_poseidon_dense", os.path.join(ROOT, "tools", "gen_poseidon_dense.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(maxsize=None)
def header_tables():
    """GLEN, POW[m][i][j] (m = 1..3, j = 1..11; index 0 unused), COL[k][i] and
    K[t][i] as Python integers, read from the committed header's text."""
    text = open(HEADER).read()
    raw = {}
    for name, body in re.findall(r"constexpr \w+ (\w+)\[\d+\] = \{(.*?)\};", text, re.S):
        raw[name] = [int(tok.rstrip("u"), 0) for tok in body.replace("\n", " ").split(",") if tok.strip()]
    glen = raw["GLEN"]
    assert len(glen) == 22 and len(raw["POW"]) == 3 * 12 * 11 and len(raw["COL"]) == 3 * 12 and len(raw["K"]) == 22 * 24
    pw = [None] + [[[0] + raw["POW"][(m * 12 + i) * 11:(m * 12 + i + 1) * 11] for i in range(12)] for m in range(3)]
    col = [raw["COL"][k * 12:(k + 1) * 12] for k in range(3)]
    K = [[raw["K"][(t * 12 + i) * 2] | raw["K"][(t * 12 + i) * 2 + 1] << 32 for i in range(12)] for t in range(22)]
    return glen, pw, col, K


def group_rows(t0, m):
    """Rows of step m (1..G) of the group starting at t0 as (coefs[i][0..10+m], k[i]):
    inputs v[1..11], x_0..x_(m-1).  Step m < G has row 0 only (y_m)."""
    glen, pw, col, K = header_tables()
    rows = range(12) if m == glen[t0] else [0]
    return ([pw[m][i][1:] + [col[m - 1 - l][i] for l in range(m)] for i in rows], [K[t0 + m - 1][i] for i in rows])


def r_dense_group(v, t0):
    """pf::dense_group<t0, GLEN[t0]> on residues, from the header's tables."""
    G = header_tables()[0][t0]
    xs = [pow(v[0], 7, P)]
    for m in range(1, G + 1):
        coefs, k = group_rows(t0, m)
        out = [(sum(c * x for c, x in zip(row, list(v[1:]) + xs)) + kk) % P for row, kk in zip(coefs, k)]
        if m < G:
            xs.append(pow(out[0], 7, P))
    return out


def r_plain_partial_rounds(v, t0, n):
    """n plain partial rounds from the state entering round 4 + t0 (constants added)."""
    g = gen()
    v = list(v)
    for r in range(4 + t0, 4 + t0 + n):
        v = [(x + c) % P for x, c in zip(g._g.matvec(g.M, [pow(v[0], 7, P)] + v[1:]), g.RC[r + 1])]
    return v


def r_permute_grouped(s):
    """permute_nc as pf::rounds<0> composes it, the groups from the header's tables."""
    g = gen()
    s = [(x + c) % P for x, c in zip(s, g.RC[0])]
    for r in range(4):
        s = [(x + c) % P for x, c in zip(g._g.matvec(g.M, [pow(x, 7, P) for x in s]), g.RC[r + 1])]
    for t0 in STARTS:
        s = r_dense_group(s, t0)
    for r in range(26, 30):
        s = g._g.matvec(g.M, [pow(x, 7, P) for x in s])
        if r < 29:
            s = [(x + c) % P for x, c in zip(s, g.RC[r + 1])]
    return s


# ---- CPU checks ---------------------------------------------------------------

def test_committed_header_is_generated():
    with open(HEADER) as f:
        assert f.read() == gen().header_text()


def test_plan():
    glen = header_tables()[0]
    assert gen().PLAN == PLAN and tuple(t for t in range(22) if glen[t]) == STARTS
    assert tuple(glen[t] for t in STARTS) == PLAN and [t0 for t0, _ in gen().group_starts()] == list(STARTS)


def test_tables_are_the_integer_powers():
    """POW[m] = (MZ)^m and COL[k] = (MZ)^k M e_0 over the integers, from M alone."""
    _, pw, col, _ = header_tables()
    Mo = np.array(gen().M, dtype=object)
    Z = np.diag([0] + [1] * 11).astype(object)
    e0 = np.array([1] + [0] * 11, dtype=object)
    MZ = Mo.dot(Z)
    acc = np.identity(12, dtype=object)
    for m in range(1, 4):
        assert col[m - 1] == acc.dot(Mo).dot(e0).tolist()
        acc = MZ.dot(acc)
        assert not acc[:, 0].any()
        assert [row[1:] for row in pw[m]] == acc[:, 1:].tolist()
    assert max(max(row) for row in pw[3]) < 1 << 22 and all(0 < c <= 64 for c in col[0])


def test_constants_are_the_pushed_round_constants():
    """K[t] = sum_(j <= m) (MZ)^(m-j) RC[4 + t0 + j] mod p, t = t0 + m - 1."""
    glen, _, _, K = header_tables()
    g = gen()
    MZ = np.array(g.M, dtype=object).dot(np.diag([0] + [1] * 11).astype(object))
    for t0 in STARTS:
        k = np.zeros(12, dtype=object)
        for m in range(1, glen[t0] + 1):
            k = MZ.dot(k) + np.array(g.RC[4 + t0 + m], dtype=object)
            assert K[t0 + m - 1] == [int(x) % P for x in k]


def test_groups_equal_plain_rounds():
    rnd = random.Random(5)
    glen = header_tables()[0]
    states = [[0] * 12, [P - 1] * 12] + [[rnd.randrange(P) for _ in range(12)] for _ in range(16)]
    for s in states:
        assert r_permute_grouped(s) == gen().permute_plain(s)
        assert gen().permute_dense_grouped(s) == gen().permute_plain(s)
        for t0 in STARTS:
            assert r_dense_group(s, t0) == r_plain_partial_rounds(s, t0, glen[t0])


REDUCE_ROW_DOMAIN = 2**60
# log2 of the worst cases with every half at 2^32 - 1, rounded up to 0.01: the
# largest integer row sum (x columns included), the largest al / ah handed to
# reduce_row, the largest t = al + eps hi32(ah) inside it
DENSE_MAXIMA_LOG2 = {"row_sum": 23.85, "acc": 55.85, "reduce_t": 56.85}


def dense_accumulator_maxima():
    worst = {"row_sum": 0, "acc": 0, "reduce_t": 0}
    glen = header_tables()[0]
    for t0 in STARTS:
        for m in range(1, glen[t0] + 1):
            for row, k in zip(*group_rows(t0, m)):
                al, ah = sum(row) * M32 + (k & M32), sum(row) * M32 + (k >> 32)
                worst["row_sum"] = max(worst["row_sum"], sum(row))
                worst["acc"] = max(worst["acc"], al, ah)
                worst["reduce_t"] = max(worst["reduce_t"], al + M32 * (ah >> 32))
    return worst


def test_accumulators_stay_in_the_tested_domain():
    assert DOMAINS["lt60"][1] == REDUCE_ROW_DOMAIN
    w = dense_accumulator_maxima()
    assert w == gen().accumulator_maxima()
    assert w["acc"] < REDUCE_ROW_DOMAIN and w["reduce_t"] < 2**64
    for name, bound in DENSE_MAXIMA_LOG2.items():
        assert bound - 0.01 <= math.log2(w[name]) < bound, (name, math.log2(w[name]))


def test_mad_count():
    """two mads per term: 2 988 for the shipped plan"""
    glen = header_tables()[0]
    n = sum(2 * len(row) for t0 in STARTS for m in range(1, glen[t0] + 1) for row in group_rows(t0, m)[0])
    assert n == gen().mad_count() == 2988


# ---- the step model of pf::dense_group and its state set ----------------------

def group_model(s, t0):
    """Raw words of pf::dense_group<t0, G> on raw states s[n][12], and the
    reduce_row paths of the output rows [n][12] and of y_1..y_(G-1) [n][G-1]:
    x_0 = sbox(s_0); every row the exact al, ah over the 32-bit halves of
    v[1..11] and x_l, seeded with the halves of K, then reduce_row."""
    G = header_tables()[0][t0]
    with np.errstate(over="ignore"):
        lo, hi = halves(np.ascontiguousarray(s[:, 1:]))
        xl, xh = halves(raw_sbox(np.ascontiguousarray(s[:, 0])))
        lo, hi = np.column_stack([lo, xl]), np.column_stack([hi, xh])
        ypaths = []
        for m in range(1, G + 1):
            coefs, k = group_rows(t0, m)
            Ct = np.array(coefs, dtype=np.uint64).T
            k = np.array(k, dtype=np.uint64)
            al, ah = lo @ Ct + (k & U(M32)), hi @ Ct + (k >> U(32))
            assert int(al.max()) < REDUCE_ROW_DOMAIN and int(ah.max()) < REDUCE_ROW_DOMAIN
            raw, path = m_reduce_row(al, ah)
            if m < G:
                ypaths.append(path[:, 0])
                xl, xh = halves(raw_sbox(np.ascontiguousarray(raw[:, 0])))
                lo, hi = np.column_stack([lo, xl]), np.column_stack([hi, xh])
    return raw, path, np.column_stack(ypaths)


NSEARCH = {3: 1 << 14, 2: 1 << 19}  # candidates of the carry search per group length


@functools.lru_cache(maxsize=None)
def carry_states(t0):
    """States that take reduce_row's carry: one for y_1 and one per output row.

    y_1 reads free inputs (v[1..11] and x_0 = v_0^7), so carry_targets' closed
    form applies with M's row 0 and K.  The later rows also read x_1 (x_2),
    S-box outputs of the state's own earlier rows, so no closed form fixes
    lo32(ah); with every half of v[1..11] at 2^32 - 1 (the largest hi32(t)) a
    row carries for about row_sum / 2^31 of the v_0, and the first carrying
    v_0 of a seeded sequence is taken, found with the exact step model."""
    g = gen()
    y1 = carry_targets(g.M, [header_tables()[3][t0][0]] + [0] * 11)[0]
    first = [pow(y1[0], INV7, P)] + y1[1:]
    G = header_tables()[0][t0]
    cand = np.full((NSEARCH[G], 12), (1 << 64) - 1, np.uint64)
    cand[:, 0] = np.random.default_rng(0xD6 + t0).integers(0, 1 << 64, NSEARCH[G], dtype=np.uint64)
    _, path, _ = group_model(cand, t0)
    assert (path & U(1)).any(axis=0).all(), f"group {t0}: a row without a carrying candidate"
    picks = [int(np.argmax(path[:, i] & U(1))) for i in range(12)]
    out = np.concatenate([np.array([first], dtype=np.uint64), cand[picks]])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def group_states(t0):
    """state_set("u64") (edge states, 2^10 uniform), then the carry states."""
    s = np.concatenate([state_set("u64")[0], carry_states(t0)])
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("t0", STARTS)
def test_state_set_takes_both_carries(t0):
    """Every output row, and y_1, takes reduce_row's carry and its no-carry
    path somewhere in the group's state set, and never a step documented as
    impossible."""
    _, path, ypaths = group_model(group_states(t0), t0)
    assert not (path & U(0b110)).any() and not (ypaths & U(0b110)).any(), "reduce_row wraps"
    for lane in range(12):
        assert set(np.unique(path[:, lane]).tolist()) == {0, 1}, f"group {t0}: row {lane} misses a carry value"
    assert set(np.unique(ypaths[:, 0]).tolist()) == {0, 1}, f"group {t0}: y_1 misses a carry value"


@pytest.mark.parametrize("t0", STARTS)
def test_group_model_agrees_with_integers(t0):
    s = group_states(t0)
    assert canon_rows(group_model(s, t0)[0]) == [r_dense_group(v, t0) for v in canon_rows(s)]
