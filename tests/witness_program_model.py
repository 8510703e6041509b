"""A builder of small witness-generator programs and a Python-integer model of
them (test infrastructure for test_witness_program_model.py and
test_gpu_witness_program.py).

The device runs a circuit's witness generators from a table of 40-byte records
grouped into dependency levels (csrc/circuit.h DevGen, csrc/witness.hip).  The
builder here lays out gate rows and free value slots by hand, emits records in
levels, finds each level's Poseidon run and flags the slots with several
writers (DEV_MULTI), so a test can put any kind at any value in any schedule.
The model executes the same program level by level over Python integers, every
kind restated from its generator's definition: products, Horner accumulation,
bit splits, a list lookup, the extension-field quotient, the MDS layer, the
value at a point of the polynomial interpolating a coset (by Lagrange's
formula) and a round-by-round Poseidon.  It yields the slot values, or the set
of generator indices that fail.

Failure model.  A generator fails at its root cause (an unset input, a zero
divisor, an index of 16 or more, a shift of zero, a set bit under the zero
slot, a conflicting write).  What a failed generator would have written is
tainted, and a generator that touches a tainted or unset slot fails in turn:
`failed` is the root causes and everything downstream, `first` the failures of
the earliest level that has any.
"""
import numpy as np

from test_recursion_gates import MDS_CIRC, eadd, emul, escale, esub, inv, mds, root  # noqa: F401

P = 0xFFFFFFFF00000001
UNSET = (1 << 64) - 1
MULTI = 1 << 31
W = 135

(CONSTANT, ARITH, POSEIDON, BASE_SPLIT, EQUALITY, WIRE_SPLIT, EXT_DIV, RANDOM_ACCESS, ARITH_EXT, MUL_EXT, REDUCING,
 REDUCING_EXT, POSEIDON_MDS, COSET_INTERP) = range(14)
KIND_NAMES = ["CONSTANT", "ARITH", "POSEIDON", "BASE_SPLIT", "EQUALITY", "WIRE_SPLIT", "EXT_DIV", "RANDOM_ACCESS",
              "ARITH_EXT", "MUL_EXT", "REDUCING", "REDUCING_EXT", "POSEIDON_MDS", "COSET_INTERP"]
RED_COEFFS, REDE_COEFFS = 43, 32
# CosetInterpolationGate{4, 6}: shift 0, values 1.., evaluation point, value, intermediates, shifted point
CI_POINTS, CI_DEGREE, CI_NINT = 16, 6, 2
CI_EVAL_POINT, CI_EVAL_VALUE, CI_INTER, CI_SHIFTED = 33, 35, 37, 45
# PoseidonGate wires: input 0.., output 12.., swap 24, delta 25.., first full rounds' S-box inputs 29..,
# partial rounds' 65.., second full rounds' 87..
PG_OUT, PG_SWAP, PG_DELTA, PG_FULL0, PG_PARTIAL, PG_FULL1 = 12, 24, 25, 29, 65, 87


def poseidon_constants():
    """The round constants and MDS matrix, from where test_gpu_poseidon_forms takes them."""
    from test_gpu_poseidon_forms import gen
    return gen().RC, gen().M


def poseidon_row(inp, swap):
    """{wire: value} of a PoseidonGate row with the given inputs: the plain
    permutation round by round, each S-box input a wire."""
    RC, M = poseidon_constants()
    w = {}
    s = list(inp)
    for i in range(4):
        w[PG_DELTA + i] = swap * (s[i + 4] - s[i]) % P
    if swap == 1:
        s[0:4], s[4:8] = s[4:8], s[0:4]
    for r in range(30):
        s = [(x + c) % P for x, c in zip(s, RC[r])]
        if r < 4 or r >= 26:
            if 1 <= r < 4:
                w.update({PG_FULL0 + 12 * (r - 1) + i: s[i] for i in range(12)})
            if r >= 26:
                w.update({PG_FULL1 + 12 * (r - 26) + i: s[i] for i in range(12)})
            s = [pow(x, 7, P) for x in s]
        else:
            w[PG_PARTIAL + r - 4] = s[0]
            s[0] = pow(s[0], 7, P)
        s = [sum(a * x for a, x in zip(row, s)) % P for row in M]
    w.update({PG_OUT + i: s[i] for i in range(12)})
    return w


def ext_div(num, den):
    """(a + bX) / (c + dX), X^2 = 7."""
    norm = (den[0] * den[0] - 7 * den[1] * den[1]) % P
    return escale(emul(num, (den[0], (-den[1]) % P)), inv(norm))


def coset_interp_row(shift, vals, z):
    """{wire: value} of the InterpolationGenerator's outputs: the value by
    Lagrange's formula over the coset, the intermediates by the chunked fold."""
    w = {}
    pt = escale(z, inv(shift))
    w[CI_SHIFTED], w[CI_SHIFTED + 1] = pt
    om = root(4)
    xs = [shift * pow(om, i, P) % P for i in range(CI_POINTS)]
    acc = (0, 0)
    for i in range(CI_POINTS):
        num, den = (1, 0), 1
        for j in range(CI_POINTS):
            if j != i:
                num = emul(num, esub(z, (xs[j], 0)))
                den = den * (xs[i] - xs[j]) % P
        acc = eadd(acc, escale(emul(vals[i], num), inv(den)))
    w[CI_EVAL_VALUE], w[CI_EVAL_VALUE + 1] = acc
    n_inv = inv(CI_POINTS)
    e, p = (0, 0), (1, 0)
    lo, hi = 0, CI_DEGREE
    for it in range(CI_NINT + 1):
        for i in range(lo, hi):
            x = pow(om, i, P)
            t = esub(pt, (x, 0))
            e = eadd(emul(e, t), emul(escale(vals[i], x * n_inv % P), p))
            p = emul(p, t)
        if it == CI_NINT:
            break
        w[CI_INTER + 2 * it], w[CI_INTER + 2 * it + 1] = e
        w[CI_INTER + 2 * (CI_NINT + it)], w[CI_INTER + 2 * (CI_NINT + it) + 1] = p
        lo = 1 + (CI_DEGREE - 1) * (it + 1)
        hi = min(lo + CI_DEGREE - 1, CI_POINTS)
    assert e == acc  # the fold is the interpolant
    return w


class Gen:
    __slots__ = ("kind", "row", "s", "k0", "k1")

    def __init__(self, kind, row=0, s=(), k0=0, k1=0):
        self.kind, self.row, self.k0, self.k1 = kind, row, k0, k1
        self.s = list(s) + [0] * (4 - len(s))


class Program:
    """Gate rows, free slots, inputs and generator records in levels."""

    def __init__(self, limbs=63, num_consts=2):
        self.limbs, self.num_consts = limbs, num_consts
        self.nslots = 1  # slot 0: the shared never-set slot (value 0)
        self.rows = []   # [row][wire] -> slot
        self.levels = [[]]
        self.in_slots = []
        self.zero_slot = 0

    # ---- layout
    def slot(self):
        self.nslots += 1
        return self.nslots - 1

    def slots(self, n):
        return [self.slot() for _ in range(n)]

    def input(self):
        s = self.slot()
        self.in_slots.append(s)
        return s

    def inputs(self, n):
        return [self.input() for _ in range(n)]

    def row(self, wires=None):
        """a new gate row; wires: {wire: slot} placed as given, the rest fresh slots"""
        wires = wires or {}
        self.rows.append([wires[j] if j in wires else self.slot() for j in range(W)])
        return len(self.rows) - 1

    def input_row(self, cols):
        """a new row whose wires `cols` are inputs"""
        return self.row({j: self.input() for j in cols})

    def wire(self, row, j):
        return self.rows[row][j]

    # ---- records
    def level(self):
        self.levels.append([])

    def emit(self, kind, row=0, s=(), k0=0, k1=0):
        self.levels[-1].append(Gen(kind, row, s, k0, k1))
        return sum(len(lv) for lv in self.levels) - 1

    def gens(self):
        return [g for lv in self.levels for g in lv]

    # ---- what a record reads and writes (slots)
    def reads_writes(self, g):
        k = g.kind
        ws = self.rows[g.row] if k not in (CONSTANT, ARITH, EQUALITY, EXT_DIV) else None
        if k == CONSTANT:
            return [], g.s[:1 if self.num_consts < 2 else 2]
        if k == ARITH:
            return g.s[:3], [g.s[3]]
        if k == EQUALITY:
            return g.s[:2], g.s[2:4]
        if k == EXT_DIV:
            return g.s[:4], [g.k0 & 0xFFFFFFFF, g.k0 >> 32]
        if k == BASE_SPLIT:
            return [g.s[0]], [ws[1 + i] for i in range(self.limbs) if not (self.zero_slot and ws[1 + i] == self.zero_slot)]
        if k == WIRE_SPLIT:
            return [g.s[0]], [self.rows[g.row + j][0] for j in range(g.s[1])]
        if k == RANDOM_ACCESS:
            c = g.s[0]
            return ([ws[18 * c]] + [ws[18 * c + 2 + i] for i in range(16)],
                    [ws[18 * c + 1]] + [ws[74 + 4 * c + i] for i in range(4)])
        if k == ARITH_EXT:
            o = 8 * g.s[0]
            return ws[o:o + 6], ws[o + 6:o + 8]
        if k == MUL_EXT:
            o = 6 * g.s[0]
            return ws[o:o + 4], ws[o + 4:o + 6]
        if k in (REDUCING, REDUCING_EXT):
            nc, cw = (RED_COEFFS, 1) if k == REDUCING else (REDE_COEFFS, 2)
            return ws[2:6 + cw * nc], ws[0:2] + ws[6 + cw * nc:6 + cw * nc + 2 * (nc - 1)]
        if k == POSEIDON_MDS:
            return ws[0:24], ws[24:48]
        if k == COSET_INTERP:
            return ws[0:CI_EVAL_POINT + 2], ws[CI_EVAL_VALUE:CI_SHIFTED + 2]
        if k == POSEIDON:
            return ws[0:12] + [ws[PG_SWAP]], ws[12:24] + ws[25:135]
        raise ValueError(k)

    # ---- the device tables
    def multi_slots(self):
        """slots with more than one writer (an input counts as one), and the zero slot"""
        n = {}
        for s in self.in_slots:
            n[s] = n.get(s, 0) + 1
        for g in self.gens():
            for s in self.reads_writes(g)[1]:
                n[s] = n.get(s, 0) + 1
        m = {s for s, c in n.items() if c > 1}
        if self.zero_slot:
            m.add(self.zero_slot)
        return m

    def tables(self):
        """(gens [n][5] u64, level_off, level_pos [nlevels][2], wslot [nrows][W]) as the device takes them"""
        multi = self.multi_slots()

        def f(s):
            return s | MULTI if s in multi else s
        recs = []
        for g in self.gens():
            s = list(g.s)
            nsl = {CONSTANT: 2, ARITH: 4, EQUALITY: 4, EXT_DIV: 4, BASE_SPLIT: 1, WIRE_SPLIT: 1}.get(g.kind, 0)
            s[:nsl] = [f(x) for x in s[:nsl]]
            k0 = g.k0
            if g.kind == EXT_DIV:
                k0 = f(k0 & 0xFFFFFFFF) | f(k0 >> 32) << 32
            recs.append([g.kind | g.row << 32, s[0] | s[1] << 32, s[2] | s[3] << 32, k0, g.k1])
        level_off, level_pos = [0], []
        for lv in self.levels:
            lo = level_off[-1]
            pos = [i for i, g in enumerate(lv) if g.kind == POSEIDON]
            assert not pos or pos == list(range(pos[0], pos[0] + len(pos))), "a level's Poseidon records are contiguous"
            level_pos.append([lo + pos[0] if pos else lo + len(lv), len(pos)])
            level_off.append(lo + len(lv))
        wslot = np.array([[f(s) for s in r] for r in self.rows], np.uint32).reshape(len(self.rows), W)
        return (np.array(recs, np.uint64).reshape(len(recs), 5), np.array(level_off, np.uint32),
                np.array(level_pos, np.uint32).reshape(len(self.levels), 2), wslot)


class Failed(Exception):
    pass


def run(prog, in_vals):
    """One proof: (vals[nslots], failed set, first: the failures of the earliest failing level)."""
    v = [UNSET] * prog.nslots
    v[0] = 0
    for s, x in zip(prog.in_slots, in_vals):
        v[s] = int(x)
    taint, failed, first = set(), set(), None

    def rd(s):
        if s in taint or v[s] == UNSET:
            raise Failed
        return v[s]

    def wr(s, x):
        if s in taint:
            raise Failed
        if v[s] == UNSET:
            v[s] = x
        elif v[s] != x:
            raise Failed

    def step(g):
        k, rows = g.kind, prog.rows
        ws = rows[g.row] if k not in (CONSTANT, ARITH, EQUALITY, EXT_DIV) else None

        def put(wires):
            for j, x in wires.items():
                wr(ws[j], x)
        if k == CONSTANT:
            wr(g.s[0], g.k0)
            if prog.num_consts >= 2:
                wr(g.s[1], g.k1)
        elif k == ARITH:
            wr(g.s[3], (rd(g.s[0]) * rd(g.s[1]) * g.k0 + rd(g.s[2]) * g.k1) % P)
        elif k == EQUALITY:
            x, y = rd(g.s[0]), rd(g.s[1])
            wr(g.s[2], int(x == y))
            wr(g.s[3], 0 if x == y else inv(x - y))
        elif k == EXT_DIV:
            num, den = (rd(g.s[0]), rd(g.s[1])), (rd(g.s[2]), rd(g.s[3]))
            if den == (0, 0):
                raise Failed
            q = ext_div(num, den)
            wr(g.k0 & 0xFFFFFFFF, q[0])
            wr(g.k0 >> 32, q[1])
        elif k == BASE_SPLIT:
            x = rd(g.s[0])
            bad = False
            for i in range(prog.limbs):
                bit = (x >> i) & 1
                if prog.zero_slot and ws[1 + i] == prog.zero_slot:
                    bad |= bit != 0  # checked, never written
                else:
                    wr(ws[1 + i], bit)
            if bad:
                raise Failed
        elif k == WIRE_SPLIT:
            x = rd(g.s[0])
            for j in range(g.s[1]):
                wr(rows[g.row + j][0], x & ((1 << prog.limbs) - 1))
                x >>= prog.limbs
        elif k == RANDOM_ACCESS:
            c = g.s[0]
            idx = rd(ws[18 * c])
            if idx >= 16:
                raise Failed
            wr(ws[18 * c + 1], rd(ws[18 * c + 2 + idx]))
            for i in range(4):
                wr(ws[74 + 4 * c + i], (idx >> i) & 1)
        elif k in (ARITH_EXT, MUL_EXT):
            o = (8 if k == ARITH_EXT else 6) * g.s[0]
            r = escale(emul((rd(ws[o]), rd(ws[o + 1])), (rd(ws[o + 2]), rd(ws[o + 3]))), g.k0)
            if k == ARITH_EXT:
                r = eadd(r, escale((rd(ws[o + 4]), rd(ws[o + 5])), g.k1))
            oo = o + (6 if k == ARITH_EXT else 4)
            put({oo: r[0], oo + 1: r[1]})
        elif k in (REDUCING, REDUCING_EXT):
            ext = k == REDUCING_EXT
            n, cw = (REDE_COEFFS, 2) if ext else (RED_COEFFS, 1)
            alpha, acc = (rd(ws[2]), rd(ws[3])), (rd(ws[4]), rd(ws[5]))
            coeffs = [(rd(ws[6 + 2 * i]), rd(ws[7 + 2 * i])) if ext else (rd(ws[6 + i]), 0) for i in range(n)]
            for i in range(n):
                acc = eadd(emul(acc, alpha), coeffs[i])
                o = 0 if i == n - 1 else 6 + cw * n + 2 * i
                put({o: acc[0], o + 1: acc[1]})
        elif k == POSEIDON_MDS:
            o0, o1 = mds([rd(ws[2 * i]) for i in range(12)]), mds([rd(ws[2 * i + 1]) for i in range(12)])
            for r in range(12):
                put({24 + 2 * r: o0[r], 25 + 2 * r: o1[r]})
        elif k == COSET_INTERP:
            shift = rd(ws[0])
            z = (rd(ws[CI_EVAL_POINT]), rd(ws[CI_EVAL_POINT + 1]))
            vals = [(rd(ws[1 + 2 * i]), rd(ws[2 + 2 * i])) for i in range(CI_POINTS)]
            if shift == 0:
                raise Failed
            put(coset_interp_row(shift, vals, z))
        elif k == POSEIDON:
            put(poseidon_row([rd(ws[i]) for i in range(12)], rd(ws[PG_SWAP])))
        else:
            raise ValueError(k)

    i = 0
    for lv in prog.levels:
        written, lv_failed = set(), []
        for g in lv:
            r, w = prog.reads_writes(g)
            assert not (set(r) & written), "a record reads what its own level writes"
            try:
                step(g)
            except Failed:
                failed.add(i)
                lv_failed.append(i)
                taint.update(w)
            written.update(w)
            i += 1
        # the level's writers run concurrently: a slot tainted by a later record fails the earlier ones too
        base = i - len(lv)
        for j, g in enumerate(lv):
            if base + j not in failed and (set(prog.reads_writes(g)[1]) & taint):
                failed.add(base + j)
                lv_failed.append(base + j)
        if lv_failed and first is None:
            first = sorted(lv_failed)
    return v, failed, first or []


def run_batch(prog, in_vals):
    """[B][nin] inputs -> (vals [B][nslots] u64, [failed set per proof], [first per proof])"""
    out = [run(prog, row) for row in in_vals]
    return (np.array([o[0] for o in out], np.uint64).reshape(len(out), prog.nslots), [o[1] for o in out],
            [o[2] for o in out])


def expand(prog, vals):
    """the wire matrix [W][nrows] of one proof's slot values; unset reads as 0"""
    return [[0 if vals[s] == UNSET else int(vals[s]) for s in col] for col in zip(*prog.rows)]
