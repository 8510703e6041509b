"""Generate qp-zk-circuits-rm_amd/csrc/poseidon_dense_consts.h: constants of
the small-integer grouped form of Poseidon's 22 partial rounds that the hashing
permutation (pf::rounds, poseidon_fast.h) runs.

A plain partial round is  v <- M S(v) + c,  S = x^7 on lane 0 only.  With Z
the map that zeroes lane 0, S(v) = Z v + e_0 x, x = v_0^7, so G consecutive
rounds starting from v (that round's constants already added) are

    x_0 = v_0^7
    y_m = (MZ)^m[0, 1..11] . v[1..11] + sum_(l<m) ((MZ)^(m-1-l) M e_0)[0] x_l + K_m[0],
    x_m = y_m^7                                            (m = 1 .. G-1)
    out = (MZ)^G[:, 1..11] . v[1..11] + sum_(l<G) ((MZ)^(G-1-l) M e_0) x_l + K_G
    K_m = sum_(j=1..m) (MZ)^(m-j) c_j mod p                (c_j: the constants of round j of the group + 1)

Over the integers M has entries <= 41, so for G <= 3 every coefficient is an
exact small integer (< 2^22) and a row over 32-bit halves stays below 2^56:
every term is one v_mad_u64_u32 per half, as in the dense MDS rows, and the row
reduces with the 4-instruction reduce_row.  The sparse form of
tools/gen_poseidon_partial.py pays 6 mads for a term with a full-width
constant; here 22 rounds take 2 988 mads in groups 3,3,3,3,3,3,2,2.

Tables (namespace pfd):
    GLEN[t]        length of the group that starts at partial round t, else 0
    POW[m-1][i][j-1]  (MZ)^m[i][j], m = 1..3, j = 1..11 (column 0 is zero)
    COL[k][i]      ((MZ)^k M e_0)[i], k = 0..2
    K[t][i]        32-bit halves of K_m[i] for partial round t = T0 + m - 1 of its group

    python tools/gen_poseidon_dense.py   # writes the header, self-checks

The hashing permutation runs groups of up to four (plan 4,4,4,4,3,3, tables
m = 1..4 and k = 0..3 in namespace pfd4, 2 700 mads); the pfd tables stay for
the probe's G <= 3 instances.

    python tools/gen_poseidon_dense.py --plan4   # writes poseidon_dense4_consts.h
"""
import importlib.util
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "qp-zk-circuits-rm_amd", "csrc", "poseidon_dense_consts.h")


def _partial():
    spec = importlib.util.spec_from_file_location("gen_poseidon_partial",
                                                  os.path.join(ROOT, "tools", "gen_poseidon_partial.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


_g = _partial()
P, W, M, RC = _g.P, _g.W, _g.M, _g.RC
permute_plain = _g.permute_plain

PLAN = (3, 3, 3, 3, 3, 3, 2, 2)  # partial rounds per group
GMAX = max(PLAN)
H32 = (1 << 32) - 1


def group_starts(plan=PLAN):
    """[(T0, G)]: first partial round (0..21) and length of every group."""
    out, t = [], 0
    for g in plan:
        out.append((t, g))
        t += g
    assert t == 22
    return out


def imatmul(A, B):
    """integer matrix product, no reduction"""
    return [[sum(A[i][k] * B[k][j] for k in range(W)) for j in range(W)] for i in range(W)]


def tables(gmax=GMAX):
    """POW[m] = (MZ)^m for m = 0..gmax and COL[k] = (MZ)^k M e_0 for
    k = 0..gmax-1, as exact integers."""
    MZ = [[0 if j == 0 else M[i][j] for j in range(W)] for i in range(W)]
    pw = [[[int(i == j) for j in range(W)] for i in range(W)]]
    for _ in range(gmax):
        pw.append(imatmul(MZ, pw[-1]))
    col = [[sum(pw[k][i][j] * M[j][0] for j in range(W)) for i in range(W)] for k in range(gmax)]
    return pw, col


def group_constants(t0, g, pw):
    """K_1 .. K_g (mod p) of the group starting at partial round t0."""
    out = []
    for m in range(1, g + 1):
        k = [0] * W
        for j in range(1, m + 1):
            c = RC[4 + t0 + j]
            for i in range(W):
                k[i] += sum(pw[m - j][i][q] * c[q] for q in range(W))
        out.append([x % P for x in k])
    return out


def all_constants(plan=PLAN):
    """K[t][i]: the constant of the state after partial round t of its group"""
    pw, _ = tables(max(plan))
    K = []
    for t0, g in group_starts(plan):
        K.extend(group_constants(t0, g, pw))
    assert len(K) == 22
    return K


def dense_group(v, t0, g, pw, col, K):
    """One group on residues: v enters partial round t0 with its constants
    added; returns the state entering round t0 + g."""
    xs = [pow(v[0], 7, P)]
    for m in range(1, g):
        y = sum(pw[m][0][j] * v[j] for j in range(1, W))
        y += sum(col[m - 1 - l][0] * xs[l] for l in range(m)) + K[t0 + m - 1][0]
        xs.append(pow(y % P, 7, P))
    return [(sum(pw[g][i][j] * v[j] for j in range(1, W)) + sum(col[g - 1 - l][i] * xs[l] for l in range(g)) +
             K[t0 + g - 1][i]) % P for i in range(W)]


def permute_dense_grouped(s, plan=PLAN):
    """the permutation as pf::rounds<0> composes it: full rounds 0..3, the
    partial rounds in groups, full rounds 26..29"""
    pw, col = tables(max(plan))
    K = all_constants(plan)
    s = [(x + c) % P for x, c in zip(s, RC[0])]
    for r in range(4):
        s = [(x + c) % P for x, c in zip(_g.matvec(M, [pow(x, 7, P) for x in s]), RC[r + 1])]
    for t0, g in group_starts(plan):
        s = dense_group(s, t0, g, pw, col, K)
    for r in range(26, 30):
        s = _g.matvec(M, [pow(x, 7, P) for x in s])
        if r < 29:
            s = [(x + c) % P for x, c in zip(s, RC[r + 1])]
    return s


def row_terms(m, i, pw, col):
    """coefficients of one row in the order of its inputs: v[1..11], x_0..x_(m-1)"""
    return [pw[m][i][j] for j in range(1, W)] + [col[m - 1 - l][i] for l in range(m)]


def accumulator_maxima(plan=PLAN):
    """Largest al / ah any row hands to reduce_row with every half at
    2^32 - 1, and the largest t = al + eps hi32(ah) inside it."""
    pw, col = tables(max(plan))
    K = all_constants(plan)
    worst = {"row_sum": 0, "acc": 0, "reduce_t": 0}
    for t0, g in group_starts(plan):
        for m in range(1, g + 1):
            for i in (range(W) if m == g else [0]):
                rs = sum(row_terms(m, i, pw, col))
                k = K[t0 + m - 1][i]
                al, ah = rs * H32 + (k & H32), rs * H32 + (k >> 32)
                worst["row_sum"] = max(worst["row_sum"], rs)
                worst["acc"] = max(worst["acc"], al, ah)
                worst["reduce_t"] = max(worst["reduce_t"], al + H32 * (ah >> 32))
    return worst


def mad_count(plan=PLAN):
    """v_mad_u64_u32 of the groups' rows (two per term), reduce_row not counted"""
    return sum(2 * (sum(11 + m for m in range(1, g)) + 12 * (11 + g)) for g in plan)


def header_text(plan=PLAN):
    pw, col = tables(max(plan))
    K = all_constants(plan)
    assert max(plan) <= 3 and all(c > 0 for m in range(1, max(plan) + 1) for i in range(W) for c in pw[m][i][1:])
    assert all(0 < c <= 64 for c in col[0]), "the seed term of every row takes an inline constant"
    L = []
    L.append("// poseidon_dense_consts.h -- GENERATED by tools/gen_poseidon_dense.py (see there).")
    L.append("// Poseidon-Goldilocks partial rounds in groups of up to 3 as exact small-integer rows:")
    L.append("// POW[m-1][i][j-1] = (MZ)^m[i][j], COL[k][i] = ((MZ)^k M e_0)[i], K[t][i] the pushed round")
    L.append("// constants (32-bit halves), GLEN[t] the length of the group starting at partial round t.")
    L.append("#pragma once")
    L.append("#include <stdint.h>")
    L.append("namespace pfd {")
    glen = [0] * 22
    for t0, g in group_starts(plan):
        glen[t0] = g
    L.append(f"constexpr int GLEN[22] = {{{', '.join(str(x) for x in glen)}}};")

    def arr(name, flat, per, fmt):
        L.append(f"constexpr uint32_t {name}[{len(flat)}] = {{")
        for i in range(0, len(flat), per):
            L.append("    " + ", ".join(fmt % x for x in flat[i:i + per]) + ",")
        L.append("};")

    arr("POW", [pw[m][i][j] for m in range(1, max(plan) + 1) for i in range(W) for j in range(1, W)], 11, "%du")
    arr("COL", [col[k][i] for k in range(max(plan)) for i in range(W)], 12, "%du")
    arr("K", [h for t in range(22) for i in range(W) for h in (K[t][i] & H32, K[t][i] >> 32)], 8, "0x%08xu")
    L.append("}  // namespace pfd")
    return "\n".join(L) + "\n"


# ---- groups of up to four (--plan4 -> poseidon_dense4_consts.h, namespace pfd4) ----
# (MZ)^4 has entries below 2^30 and row sums below 2^32, so a step-4 row over
# 32-bit halves reaches 2^63.8: past reduce_row's 2^60, inside reduce_row_wide's
# al < 2^64, ah < 2^64 - 2^32.  Steps 1..3 are the rows of the plan above.
HDR4 = os.path.join(ROOT, "qp-zk-circuits-rm_amd", "csrc", "poseidon_dense4_consts.h")
PLAN4 = (4, 4, 4, 4, 3, 3)  # 2 700 mads, 48 wide rows; 4,4,4,4,4,2 has 2 702 and 60
REDUCE_ROW_BOUND = 1 << 60
REDUCE_WIDE_BOUND = (1 << 64) - (1 << 32)


def row_is_wide(rs):
    """A row of integer sum rs hands reduce at most (rs + 1) (2^32 - 1) per
    accumulator (the constant's half included); the device code picks the
    reduction by the same rule (pf::dg_wide)."""
    return (rs + 1) * H32 >= REDUCE_ROW_BOUND


def accumulator_maxima4(plan=PLAN4):
    """Per reduction, the largest al / ah with every half at 2^32 - 1, the
    largest row sum and entry, and the rows (t0, m, i) that reduce wide."""
    pw, col = tables(max(plan))
    K = all_constants(plan)
    w = {"entry": 0, "row_sum": 0, "acc_row": 0, "acc_wide": 0, "wide_rows": []}
    for t0, g in group_starts(plan):
        for m in range(1, g + 1):
            for i in (range(W) if m == g else [0]):
                terms = row_terms(m, i, pw, col)
                rs, k = sum(terms), K[t0 + m - 1][i]
                acc = max(rs * H32 + (k & H32), rs * H32 + (k >> 32))
                w["entry"] = max(w["entry"], max(terms))
                w["row_sum"] = max(w["row_sum"], rs)
                if row_is_wide(rs):
                    w["acc_wide"] = max(w["acc_wide"], acc)
                    w["wide_rows"].append((t0, m, i))
                else:
                    w["acc_row"] = max(w["acc_row"], acc)
    return w


def reduce_counts(plan):
    """(rows reduced, of them wide)"""
    pw, col = tables(max(plan))
    n = nw = 0
    for _, g in group_starts(plan):
        for m in range(1, g + 1):
            for i in (range(W) if m == g else [0]):
                n += 1
                nw += row_is_wide(sum(row_terms(m, i, pw, col)))
    return n, nw


def header_text4(plan=PLAN4):
    gmax = max(plan)
    pw, col = tables(gmax)
    K = all_constants(plan)
    assert gmax == 4 and all(c > 0 for m in range(1, gmax + 1) for i in range(W) for c in pw[m][i][1:])
    assert all(0 < c <= 64 for c in col[0]), "the seed term of every row takes an inline constant"
    w = accumulator_maxima4(plan)
    assert w["entry"] < 1 << 32 and w["row_sum"] < 1 << 32, "(MZ)^4 fits 32 bits"
    assert w["acc_row"] < REDUCE_ROW_BOUND and w["acc_wide"] < REDUCE_WIDE_BOUND
    L = []
    L.append("// poseidon_dense4_consts.h -- GENERATED by tools/gen_poseidon_dense.py --plan4 (see there).")
    L.append("// Poseidon-Goldilocks partial rounds in groups of up to 4 as exact small-integer rows:")
    L.append("// POW[m-1][i][j-1] = (MZ)^m[i][j], COL[k][i] = ((MZ)^k M e_0)[i], K[t][i] the pushed round")
    L.append("// constants (32-bit halves), GLEN[t] the length of the group starting at partial round t.")
    L.append("#pragma once")
    L.append("#include <stdint.h>")
    L.append("namespace pfd4 {")
    glen = [0] * 22
    for t0, g in group_starts(plan):
        glen[t0] = g
    L.append(f"constexpr int GLEN[22] = {{{', '.join(str(x) for x in glen)}}};")

    def arr(name, flat, per, fmt):
        L.append(f"constexpr uint32_t {name}[{len(flat)}] = {{")
        for i in range(0, len(flat), per):
            L.append("    " + ", ".join(fmt % x for x in flat[i:i + per]) + ",")
        L.append("};")

    arr("POW", [pw[m][i][j] for m in range(1, gmax + 1) for i in range(W) for j in range(1, W)], 11, "%du")
    arr("COL", [col[k][i] for k in range(gmax) for i in range(W)], 12, "%du")
    arr("K", [h for t in range(22) for i in range(W) for h in (K[t][i] & H32, K[t][i] >> 32)], 8, "0x%08xu")
    L.append("}  // namespace pfd4")
    return "\n".join(L) + "\n"


def main4():
    rnd = random.Random(12)
    states = [[0] * W, [P - 1] * W] + [[rnd.randrange(P) for _ in range(W)] for _ in range(20)]
    for plan in (PLAN4, (4, 4, 4, 4, 4, 2)):
        for s in states:
            assert permute_dense_grouped(s, plan) == permute_plain(s), plan
        print("plan %s: %d mads, %d rows reduced, %d of them wide" % ((plan, mad_count(plan)) + reduce_counts(plan)))
    assert (mad_count(PLAN4), reduce_counts(PLAN4)) < (mad_count((4, 4, 4, 4, 4, 2)), reduce_counts((4, 4, 4, 4, 4, 2)))
    open(HDR4, "w").write(header_text4())
    print("dense partial-round groups %s == plain permutation; %d mads; wrote %s" % (PLAN4, mad_count(PLAN4), HDR4))


def main():
    import sys
    if "--plan4" in sys.argv[1:]:
        return main4()
    rnd = random.Random(11)
    states = [[0] * W, [P - 1] * W] + [[rnd.randrange(P) for _ in range(W)] for _ in range(20)]
    for plan in (PLAN, (3,) * 7 + (1,), (2,) * 11, (1,) * 22):
        for s in states:
            assert permute_dense_grouped(s, plan) == permute_plain(s), plan
    w = accumulator_maxima()
    assert w["acc"] < 1 << 60 and w["reduce_t"] < 1 << 64
    open(HDR, "w").write(header_text())
    print("dense partial-round groups %s == plain permutation; %d mads; wrote %s" % (PLAN, mad_count(), HDR))


if __name__ == "__main__":
    main()
