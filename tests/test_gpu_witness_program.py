"""The device witness generators (csrc/witness.hip), every kind and every
scheduler, from small hand-built programs against a Python-integer model.

Whole proofs pin the schedules three circuits happen to have, on hashes and
balances.  Here the TEST-ONLY probe qp_debug_witness_program
(csrc/witness_probe.cpp: validation, then the prover's own launches through
csrc/witness_launch.h) runs programs made by witness_program_model.Program,
and every slot value must equal the model's (witness_program_model.run, itself
held to the gate constraints by test_witness_program_model.py) word for word,
in every form, and be identical across forms.  Failing cases are defined
behaviour of the kernels: an unset read and a zero divisor are flagged, never
dereferenced.  Nothing here is meant to fault.

Forms: the four of the probe's form word, and the per-proof scheduler's
one-per-wave cooperative branch (wit_row=0 with wit_mode=0 in the prover) at
both workgroup sizes.  In the by-level forms err - 1 is exactly the failing
generator of the earliest failing level (stream order separates the levels);
in the per-proof forms every thread keeps its own first failure and any of
them may win the final compare-and-swap, so err - 1 is a member of the model's
failing set (the root cause or a generator downstream of it).

Coverage (test -> what it names):

  kind / branch                         test
  ------------------------------------  -----------------------------------------
  WG_CONSTANT (num_consts 1, 2)         test_kind_alone_constant[1|2]   
  WG_ARITH, WG_EQUALITY, WG_EXT_DIV,    test_kind_alone[<kind>] (random, the edge
  WG_WIRE_SPLIT (1 and 2 gates, limbs   cycle, and the kind's own edge tuples
  63 and 32), WG_RANDOM_ACCESS,         KIND_EDGES)
  WG_ARITH_EXT, WG_MUL_EXT,
  WG_REDUCING, WG_REDUCING_EXT (chunk
  tails 43 = 5*8+3, 32 = 4*8),
  WG_POSEIDON_MDS, WG_COSET_INTERP
  WG_BASE_SPLIT                         test_base_split (limbs 63, zero-slot limbs,
                                        bits under them clear / set / slot unset)
  WG_POSEIDON, rolled one-lane form     test_poseidon_forms[17|32|33-*] per-proof 256
                                        (count > 16), [33-*] per-proof 512 (> 32)
  WG_POSEIDON, 16-lane row form         test_poseidon_forms[*] by-level rows (all),
                                        per-proof 256 [1..16], per-proof 512 [1..32]
  WG_POSEIDON, one-wave form            test_poseidon_forms[*] by-level waves (all),
                                        per-proof wave forms below coop_max
  partly filled wave / row              counts 1, 3, 5, 15, 17, 33 (not multiples of
                                        4 / 16); exactly coop_max: 16 (256), 32 (512)
  Poseidon run not first in its level   test_poseidon_forms[*-after300]
  dependent permutations                test_poseidon_chain
  k_witness_gen 256 / 512,              every test: FORMS
  k_witness_level row=1 / row=0
  level wider than the workgroup,       test_wide_and_empty_levels (1,100 records)
  empty level
  MULTI agree / disagree / neighbour    test_multi_slots
  refusals of run_gen: unset input      test_unset_input[<kind>] (every kind that reads)
    EXT_DIV by zero                     test_refusals[ext_div_zero]
    RANDOM_ACCESS index >= 16           test_refusals[ra_index_16|ra_index_p1]
    RANDOM_ACCESS item unset            test_refusals[ra_item_unset]
    COSET_INTERP shift 0                test_refusals[coset_shift_0]
    BASE_SPLIT bit under zero slot      test_base_split[zero_set|zero_unwritten_set]
    write conflict                      test_multi_slots
  one bad proof among good neighbours   test_multi_slots, test_refusals, test_unset_input
  every kind feeding the next, B = 8    test_mixed_program
  k_witness_expand grid-stride, unset   test_expand
  -> 0, npis 0 / 1 / 300
  the probe's own validator             test_probe_refuses_malformed_programs
"""
import random

import numpy as np
import pytest

import witness_program_model as M
from edge_values import CANON_EDGES
from qp_wormhole import _native as N
from witness_program_model import P, UNSET, Program

pytestmark = pytest.mark.gpu

# (form, name, by_level): the probe's four, then the per-proof scheduler's one-per-wave branch
FORMS = [(N.WFORM_PROOF_256, "proof256", False), (N.WFORM_PROOF_512, "proof512", False),
         (N.WFORM_LEVEL_ROW, "level_row", True), (N.WFORM_LEVEL_WAVE, "level_wave", True),
         (N.WFORM_PROOF_256_WAVE, "proof256_wave", False), (N.WFORM_PROOF_512_WAVE, "proof512_wave", False)]
OM = M.root(4)


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def run_probe(ctx, form, pb, in_vals, tabs=None, **kw):
    tabs = tabs or pb.tables()
    return N.debug_witness_program(ctx, form, *tabs, pb.nslots, pb.in_slots, in_vals, limbs=pb.limbs,
                                   zero_slot=pb.zero_slot, num_consts=pb.num_consts, **kw)


def check(ctx, pb, in_vals, expect_failed=None):
    """Every form against the model: slot values of the good proofs word for
    word and identical across forms, err of the failing ones as the module
    docstring states.  expect_failed: the proofs that must fail (default none)."""
    in_vals = np.array(in_vals, np.uint64).reshape(len(in_vals), len(pb.in_slots))
    want, failed, first = M.run_batch(pb, in_vals)
    assert [b for b, f in enumerate(failed) if f] == sorted(expect_failed or []), "the case is not what it claims"
    tabs = pb.tables()
    good = [b for b, f in enumerate(failed) if not f]
    ref = None
    for form, name, by_level in FORMS:
        vals, err = run_probe(ctx, form, pb, in_vals, tabs)
        for b in range(len(in_vals)):
            if not failed[b]:
                assert err[b] == 0, (name, b, int(err[b]))
                bad = np.flatnonzero(vals[b] != want[b])
                assert bad.size == 0, (name, b, bad[:8], vals[b][bad[:8]], want[b][bad[:8]])
            elif by_level:
                assert len(first[b]) == 1 and int(err[b]) - 1 == first[b][0], (name, b, int(err[b]), first[b])
            else:
                assert int(err[b]) - 1 in failed[b], (name, b, int(err[b]), sorted(failed[b]))
        if ref is None:
            ref = vals[good]
        assert (vals[good] == ref).all(), name
    return want


def rnd_tuple(rng, m):
    return [rng.randrange(P) for _ in range(m)]


def edge_tuple(m, start):
    return [CANON_EDGES[(start + i) % len(CANON_EDGES)] for i in range(m)]


# ---- each kind alone ----------------------------------------------------------

E32, PM1 = 2**32 - 1, P - 1
CONSTS = [(PM1, PM1), (E32, E32), (1, 0), (0, 1), (0x123456789ABCDEF, PM1)]


def coset_point(shift, i):
    return (shift * pow(OM, i, P) % P, 0)


def ci_tuple(rng, shift, z):
    return [shift] + rnd_tuple(rng, 32) + list(z)


# per kind: the tuples of one instance's inputs that no real input reaches
def kind_edges(kind, rng):
    if kind == M.ARITH:
        return [[PM1, PM1, PM1], [E32, E32, E32], [PM1, E32, PM1], [E32, PM1, E32], [0, PM1, PM1], [PM1, 1, E32]]
    if kind == M.EQUALITY:
        return [[5, 4], [4, 5], [PM1, PM1], [0, PM1], [PM1, 0], [0, 0], [E32 + 1, E32], [2**63, 2**63 + 1]]
    if kind == M.WIRE_SPLIT:
        return [[2**63 + 1], [PM1], [2**63], [2**64 - 2**32 - 1], [2**63 - 1], [E32]]
    if kind == M.EXT_DIV:
        return [[PM1, PM1, 0, PM1], [PM1, E32, PM1, 0], [1, 0, 0, 1], [0, 0, E32, 0], [0, PM1, 0, 7], [3, 4, 1, 0]]
    if kind == M.RANDOM_ACCESS:
        # indices 0 and 15 in each of the 4 copies
        return [[0] + rnd_tuple(rng, 16), [15] + rnd_tuple(rng, 16), [15] + [PM1] * 16, [0] + edge_tuple(16, 3),
                [15] + edge_tuple(16, 8), [0] + [PM1] * 16, [0] + rnd_tuple(rng, 16), [15] + rnd_tuple(rng, 16)]
    if kind == M.ARITH_EXT:
        return [[PM1] * 6, [E32] * 6, [0, PM1, PM1, 0, E32, PM1]]
    if kind == M.MUL_EXT:
        return [[PM1] * 4, [E32] * 4, [0, PM1, PM1, 0]]
    if kind == M.REDUCING:
        return [[0, 0] + rnd_tuple(rng, 45), [PM1] * 47, [PM1, PM1, 0, 0] + [E32] * 43, [1, 0] + edge_tuple(45, 0)]
    if kind == M.REDUCING_EXT:
        return [[0, 0] + rnd_tuple(rng, 66), [PM1] * 68, [PM1, PM1, 0, 0] + [E32] * 64, [0, 1] + edge_tuple(66, 5)]
    if kind == M.POSEIDON_MDS:
        return [[PM1] * 24, [E32] * 24, [0] * 24, edge_tuple(24, 9)]
    if kind == M.COSET_INTERP:
        # the evaluation point on the coset (one term zero): first point, both chunk boundaries, last point
        out = [ci_tuple(rng, sh, coset_point(sh, i)) for sh, i in [(7, 0), (PM1, 5), (E32, 6), (3, 10), (2**63, 11),
                                                                      (1, 15)]]
        return out + [[PM1] * 35, [1] + [0] * 34]
    raise ValueError(kind)


def kind_program(kind, variant=0):
    """(program, inputs per instance, instances, fix(tuple)): 3-5 instances of `kind` in one level"""
    pb = Program(limbs=32 if (kind, variant) == (M.WIRE_SPLIT, 1) else 63)
    fix = None
    if kind == M.ARITH:
        for k in range(5):
            a, b, c = pb.inputs(3)
            pb.emit(kind, 0, [a, b, c, pb.slot()], *CONSTS[k])
        return pb, 3, 5, fix
    if kind == M.EQUALITY:
        for k in range(4):
            x, y = pb.inputs(2)
            pb.emit(kind, 0, [x, y, pb.slot(), pb.slot()])
        return pb, 2, 4, fix
    if kind == M.WIRE_SPLIT:
        for k in range(4):  # over 1 and 2 gates
            x = pb.input()
            n = 1 + k % 2
            r = [pb.row() for _ in range(n)][0]
            pb.emit(kind, r, [x, n])
        return pb, 1, 4, fix
    if kind == M.EXT_DIV:
        for k in range(4):
            s = pb.inputs(4)
            pb.emit(kind, 0, s, pb.slot() | pb.slot() << 32)

        def fix(t):
            t[2] = t[2] or 1
        return pb, 4, 4, fix
    if kind == M.RANDOM_ACCESS:
        r = pb.input_row([18 * c + j for c in range(4) for j in [0] + list(range(2, 18))])
        for c in range(4):
            pb.emit(kind, r, [c])

        def fix(t):
            t[0] %= 16
        return pb, 17, 4, fix
    if kind in (M.ARITH_EXT, M.MUL_EXT):
        ops, w, nin = ((0, 4, 9), 8, 6) if kind == M.ARITH_EXT else ((0, 5, 12), 6, 4)
        r = pb.input_row([w * i + j for i in ops for j in range(nin)])
        for k, i in enumerate(ops):
            pb.emit(kind, r, [i], *CONSTS[k if variant == 0 else k + 2])
        return pb, nin, 3, fix
    if kind in (M.REDUCING, M.REDUCING_EXT):
        n = 6 + (43 if kind == M.REDUCING else 64)
        for k in range(3):
            pb.emit(kind, pb.input_row(range(2, n)))
        return pb, n - 2, 3, fix
    if kind == M.POSEIDON_MDS:
        for k in range(3):
            pb.emit(kind, pb.input_row(range(24)))
        return pb, 24, 3, fix
    if kind == M.COSET_INTERP:
        for k in range(3):
            pb.emit(kind, pb.input_row(range(35)))

        def fix(t):
            t[0] = t[0] or 1
        return pb, 35, 3, fix
    raise ValueError(kind)


KIND_CASES = [(k, v) for k in (M.ARITH, M.EQUALITY, M.WIRE_SPLIT, M.EXT_DIV, M.RANDOM_ACCESS, M.ARITH_EXT, M.MUL_EXT,
                               M.REDUCING, M.REDUCING_EXT, M.POSEIDON_MDS, M.COSET_INTERP)
              for v in ((0, 1) if k in (M.WIRE_SPLIT, M.ARITH_EXT, M.MUL_EXT) else (0,))]


def kind_inputs(kind, pb, m, ninst, fix, rng):
    """proofs: random, two edge cycles, then the kind's edge tuples, `ninst` per proof (at most 8 proofs)"""
    def fixed(t):
        if fix:
            fix(t)
        return t
    proofs = [[fixed(rnd_tuple(rng, m)) for _ in range(ninst)],
              [fixed(edge_tuple(m, 5 * i)) for i in range(ninst)],
              [fixed(edge_tuple(m, 11 + 3 * i)) for i in range(ninst)]]
    edges = kind_edges(kind, rng)
    while edges:
        row, edges = edges[:ninst], edges[ninst:]
        proofs.append(row + [fixed(rnd_tuple(rng, m)) for _ in range(ninst - len(row))])
    assert len(proofs) <= 8
    return [[x for t in p for x in t] for p in proofs]


@pytest.mark.parametrize("kind,variant", KIND_CASES, ids=[f"{M.KIND_NAMES[k]}-{v}" for k, v in KIND_CASES])
def test_kind_alone(ctx, kind, variant):
    rng = random.Random(1000 + 10 * kind + variant)
    pb, m, ninst, fix = kind_program(kind, variant)
    check(ctx, pb, kind_inputs(kind, pb, m, ninst, fix, rng))


@pytest.mark.parametrize("num_consts", [1, 2])
def test_kind_alone_constant(ctx, num_consts):
    pb = Program(num_consts=num_consts)
    second = []
    for k0, k1 in CONSTS:
        a, b = pb.slot(), pb.slot()
        second.append(b)
        pb.emit(M.CONSTANT, 0, [a, b], k0, k1)
    want = check(ctx, pb, np.zeros((2, 0), np.uint64))
    # with one constant per gate the second slot is never written
    assert all((want[0][b] == UNSET) == (num_consts == 1) for b in second)


BASE_SPLIT_CASES = ["no_zero", "zero_clear", "zero_set", "zero_unwritten_clear", "zero_unwritten_set"]


@pytest.mark.parametrize("case", BASE_SPLIT_CASES)
def test_base_split(ctx, case):
    """limbs = 63; sums with bit 63 set; limbs wired to the zero slot are
    checked, not written: bits under them clear in one case and set in another
    (a refusal).  zero_unwritten: the zero slot still unset when the generator
    runs, so a compare that missed it would write it."""
    rng = random.Random(len(case))
    pb = Program()
    zero_wires = []
    if case != "no_zero":
        pb.zero_slot = pb.input() if "unwritten" not in case else pb.slot()
        zero_wires = [1 + i for i in (0, 31, 32, 40, 62)]
    rows = []
    for k in range(4):
        r = pb.row({j: pb.zero_slot for j in zero_wires})
        rows.append(r)
        pb.rows[r][0] = pb.input()
        pb.emit(M.BASE_SPLIT, r, [pb.wire(r, 0)])
    clear = ~sum(1 << (j - 1) for j in zero_wires)
    sums = [[2**63 + 5, PM1, 2**63, rng.randrange(P)], [rng.randrange(P) for _ in range(4)], [E32, 2**63 - 1, 0, 1],
            edge_tuple(4, 9)]
    sums = [[s & clear for s in row] for row in sums]
    expect = []
    if case.endswith("_set"):
        sums[1][2] |= 1 << 31  # one generator of one proof has a bit under the zero slot
        sums[1][2] %= P
        expect = [1]
    zin = [0] if case in ("zero_clear", "zero_set") else []
    want = check(ctx, pb, [zin + row for row in sums], expect)
    if "unwritten" in case:
        assert want[0][pb.zero_slot] == UNSET


# ---- Poseidon forms --------------------------------------------------------------

def poseidon_level(pb, n):
    rows = [pb.input_row(list(range(12)) + [M.PG_SWAP]) for _ in range(n)]
    for r in rows:
        pb.emit(M.POSEIDON, r)
    return rows


def poseidon_inputs(rng, n, lead):
    """4 proofs: random states under two complementary swap patterns, all P - 1, all 0"""
    out = []
    for b in range(4):
        row = rnd_tuple(rng, lead)
        for i in range(n):
            state = rnd_tuple(rng, 12) if b < 2 else [PM1] * 12 if b == 2 else [0] * 12
            row += state + [(i + b) & 1]
        out.append(row)
    return out


# which case reaches which form (coop_max = 16 at 256 threads, 32 at 512):
#   rolled one-lane form: per-proof 256 at 17, 32, 33; per-proof 512 at 33
#   16-lane row form:     by-level rows at every count; per-proof 256 at 1..16; per-proof 512 at 1..32
#   one-wave form:        by-level waves at every count; per-proof wave forms at and below coop_max
POSEIDON_COUNTS = [1, 3, 4, 5, 15, 16, 17, 32, 33]


def test_poseidon_counts_reach_every_form():
    for threads in (256, 512):
        cm = 4 * (threads // 64)
        assert cm in POSEIDON_COUNTS and cm + 1 in POSEIDON_COUNTS          # both sides of coop_max
        assert any(n <= cm for n in POSEIDON_COUNTS) and any(n > cm for n in POSEIDON_COUNTS)
    assert any(n % 4 for n in POSEIDON_COUNTS) and any(n % 16 for n in POSEIDON_COUNTS)


@pytest.mark.parametrize("where", ["first", "after300"])
@pytest.mark.parametrize("n", POSEIDON_COUNTS)
def test_poseidon_forms(ctx, n, where):
    rng = random.Random(50 * n + len(where))
    pb = Program()
    lead = 0
    if where == "after300":  # the Poseidon run does not start its level
        a, b, c = pb.inputs(3)
        lead = 3
        for k in range(300):
            pb.emit(M.ARITH, 0, [a, b, c, pb.slot()], k + 1, PM1 - k)
    poseidon_level(pb, n)
    check(ctx, pb, poseidon_inputs(rng, n, lead))


def test_poseidon_chain(ctx):
    """three dependent permutations, one level each; two chains side by side"""
    rng = random.Random(77)
    pb = Program()
    prev = poseidon_level(pb, 2)
    for _ in range(2):
        pb.level()
        nxt = []
        for r in prev:
            wires = {i: pb.wire(r, M.PG_OUT + i) for i in range(12)}
            wires[M.PG_SWAP] = pb.input()
            nxt.append(pb.row(wires))
            pb.emit(M.POSEIDON, nxt[-1])
        prev = nxt
    ins = [[x for i in range(2) for x in rnd_tuple(rng, 12) + [(i + b) & 1]] + [(b >> k) & 1 for k in range(4)]
           for b in range(4)]
    check(ctx, pb, ins)


# ---- conflicts and refusals ---------------------------------------------------------

def test_multi_slots(ctx):
    """x has two writers in different levels and y two in one level (which
    agree); z, allocated between them, has one.  Proof 2's writers of x
    disagree: it alone fails, at the second writer."""
    pb = Program()
    a, b, c = pb.inputs(3)
    x, z, y, t = pb.slots(4)
    pb.emit(M.ARITH, 0, [a, b, a, x], 1, 0)   # x = a b
    pb.emit(M.ARITH, 0, [a, a, b, z], 1, 1)   # z = a^2 + b
    pb.emit(M.ARITH, 0, [a, b, b, y], 2, 0)   # y = 2 a b, twice in this level
    pb.emit(M.ARITH, 0, [b, a, a, y], 2, 0)
    pb.level()
    pb.emit(M.ARITH, 0, [a, a, c, x], 0, 1)   # x = c
    pb.level()
    pb.emit(M.ARITH, 0, [z, y, a, t], 1, 1)
    assert pb.multi_slots() == {x, y}
    ins = [[3, 5, 15], [PM1, PM1, 1], [3, 5, 16], [E32, E32 + 2, (E32 * (E32 + 2)) % P]]
    check(ctx, pb, ins, expect_failed=[2])


def refusal_program(case):
    rng = random.Random(len(case))
    pb = Program()
    if case == "ext_div_zero":
        for k in range(3):
            pb.emit(M.EXT_DIV, 0, pb.inputs(4), pb.slot() | pb.slot() << 32)
        ins = [rnd_tuple(rng, 12) for _ in range(3)]
        ins[1][4:8] = [PM1, 5, 0, 0]
    elif case.startswith("ra_"):
        r = pb.input_row([18 * c + j for c in range(4) for j in [0] + list(range(2, 18))])
        if case == "ra_item_unset":  # copy 2's item 9 is a slot nobody writes
            pb.in_slots.remove(pb.wire(r, 18 * 2 + 2 + 9))
        for c in range(4):
            pb.emit(M.RANDOM_ACCESS, r, [c])
        at = [pb.in_slots.index(pb.wire(r, 18 * c)) for c in range(4)]  # the copies' index inputs
        ins = [rnd_tuple(rng, len(pb.in_slots)) for _ in range(3)]
        for row in ins:
            for c in range(4):
                row[at[c]] = rng.randrange(16)
        if case == "ra_item_unset":
            ins[0][at[2]], ins[1][at[2]], ins[2][at[2]] = 8, 9, 10
        else:
            ins[1][at[1]] = 16 if case == "ra_index_16" else PM1
    elif case == "coset_shift_0":
        for k in range(2):
            pb.emit(M.COSET_INTERP, pb.input_row(range(35)))
        ins = [rnd_tuple(rng, 70) for _ in range(3)]
        ins[1][35] = 0
    return pb, ins


@pytest.mark.parametrize("case", ["ext_div_zero", "ra_index_16", "ra_index_p1", "ra_item_unset", "coset_shift_0"])
def test_refusals(ctx, case):
    """the middle proof of three is refused; its neighbours are correct in every slot"""
    pb, ins = refusal_program(case)
    check(ctx, pb, ins, expect_failed=[1])


UNSET_KINDS = [M.ARITH, M.POSEIDON, M.BASE_SPLIT, M.EQUALITY, M.WIRE_SPLIT, M.EXT_DIV, M.RANDOM_ACCESS, M.ARITH_EXT,
               M.MUL_EXT, M.REDUCING, M.REDUCING_EXT, M.POSEIDON_MDS, M.COSET_INTERP]


@pytest.mark.parametrize("kind", UNSET_KINDS, ids=[M.KIND_NAMES[k] for k in UNSET_KINDS])
def test_unset_input(ctx, kind):
    """An input of the middle proof arrives unset (2^64 - 1): the one generator
    that reads it fails, in that proof only.  The last input of the second
    instance: for the row kinds the last value the generator loads."""
    rng = random.Random(300 + kind)
    if kind == M.POSEIDON:
        pb, m, ninst, fix = Program(), 13, 3, None
        poseidon_level(pb, 3)
    elif kind == M.BASE_SPLIT:
        pb, m, ninst, fix = Program(), 1, 3, None
        for k in range(3):
            r = pb.input_row([0])
            pb.emit(kind, r, [pb.wire(r, 0)])
    else:
        pb, m, ninst, fix = kind_program(kind)
    ins = []
    for b in range(3):
        row = []
        for i in range(ninst):
            t = rnd_tuple(rng, m)
            if kind == M.POSEIDON:
                t[12] &= 1
            if fix:
                fix(t)
            row += t
        ins.append(row)
    # RANDOM_ACCESS reads one item only: its index input instead
    ins[1][m if kind == M.RANDOM_ACCESS else 2 * m - 1] = UNSET
    check(ctx, pb, ins, expect_failed=[1])


# ---- wide and empty levels, a mixed program -----------------------------------------

def test_wide_and_empty_levels(ctx):
    """1,100 ARITH records in one level (more than two strides of a 512-thread
    workgroup, five blocks by level), an empty level, then readers of the wide
    level's first, last and stride-boundary outputs"""
    rng = random.Random(11)
    pb = Program()
    ins = pb.inputs(7)
    outs = pb.slots(1100)
    for k, o in enumerate(outs):
        pb.emit(M.ARITH, 0, [ins[k % 7], ins[(k + 1) % 7], ins[(k + 3) % 7], o], k + 1, PM1 - k)
    pb.level()
    pb.level()
    for k in (0, 255, 256, 511, 512, 1023, 1024, 1099):
        pb.emit(M.ARITH, 0, [outs[k], outs[1099 - k], ins[0], pb.slot()], 1, 1)
    assert [len(lv) for lv in pb.levels] == [1100, 0, 8]
    check(ctx, pb, [rnd_tuple(rng, 7), edge_tuple(7, 12), [PM1] * 7])


def mixed_program():
    pb = Program()
    a, b, bit = pb.inputs(3)
    c0, c1, x = pb.slots(3)
    pb.emit(M.CONSTANT, 0, [c0, c1], 6, PM1)
    pb.emit(M.ARITH, 0, [a, b, a, x], 1, 0)                                   # x = a b
    pb.level()
    eq, ivs = pb.slots(2)
    pb.emit(M.EQUALITY, 0, [x, c0, eq, ivs])
    pos = pb.row({0: x, 1: c1, **{i: pb.input() for i in range(2, 12)}, M.PG_SWAP: bit})
    pb.emit(M.POSEIDON, pos)
    pb.level()
    q0, q1 = pb.slots(2)
    pb.emit(M.EXT_DIV, 0, [pb.wire(pos, 12), pb.wire(pos, 13), x, ivs], q0 | q1 << 32)
    s0, s1 = pb.row(), pb.row()
    pb.emit(M.WIRE_SPLIT, s0, [pb.wire(pos, 14), 2])
    pb.level()
    for r in (s0, s1):
        pb.emit(M.BASE_SPLIT, r, [pb.wire(r, 0)])
    ae = pb.row({0: q0, 1: q1, 2: pb.wire(pos, 15), 3: pb.wire(pos, 16), 4: c1, 5: pb.input()})
    pb.emit(M.ARITH_EXT, ae, [0], PM1, E32)
    pb.level()
    ra = pb.row({0: eq, **{2 + i: pb.wire(pos, 29 + i) for i in range(16)}})
    pb.emit(M.RANDOM_ACCESS, ra, [0])
    me = pb.row({6 * 12 + 0: pb.wire(ae, 6), 6 * 12 + 1: pb.wire(ae, 7), 6 * 12 + 2: q0, 6 * 12 + 3: q1})
    pb.emit(M.MUL_EXT, me, [12], 3)
    pb.level()
    red = pb.row({2: pb.wire(me, 76), 3: pb.wire(me, 77), 4: pb.wire(ae, 6), 5: pb.wire(ra, 1),
                  **{6 + i: pb.wire(pos, 29 + i) for i in range(43)}})
    pb.emit(M.REDUCING, red)
    rede = pb.row({2: q0, 3: q1, 4: pb.wire(s0, 0), 5: pb.wire(s1, 0),
                   **{6 + i: pb.wire(pos, 65 + i) for i in range(64)}})
    pb.emit(M.REDUCING_EXT, rede)
    pb.level()
    mdsr = pb.row({i: pb.wire(red, 49 + i) for i in range(24)})
    pb.emit(M.POSEIDON_MDS, mdsr)
    ci = pb.row({0: x, **{1 + i: pb.wire(rede, 70 + i) for i in range(32)}, 33: pb.wire(red, 0), 34: pb.wire(red, 1)})
    pb.emit(M.COSET_INTERP, ci)
    pb.level()
    last = pb.row({**{i: pb.wire(mdsr, 24 + 2 * i) for i in range(12)}, M.PG_SWAP: eq})
    pb.emit(M.POSEIDON, last)
    return pb


def test_mixed_program(ctx):
    """one row of every kind, each fed by earlier ones, over 8 levels; 8 proofs
    with different inputs (proof 3: the EQUALITY holds)"""
    rng = random.Random(8)
    pb = mixed_program()
    assert sorted({g.kind for g in pb.gens()}) == list(range(14)) and len(pb.levels) >= 6
    ins = [[rng.randrange(1, P), rng.randrange(1, P), b & 1] + rnd_tuple(rng, len(pb.in_slots) - 3) for b in range(8)]
    ins[3][0:2] = [2, 3]
    ins[5][0:2] = [PM1, PM1]
    check(ctx, pb, ins)


# ---- expand ----------------------------------------------------------------------

def test_expand(ctx):
    """nrows = 2048: 135 * 2048 wires exceed 1024 * 256, the grid-stride branch
    of k_witness_expand.  Unset slots read as 0; public inputs for npis 0, 1, 300."""
    rng = random.Random(2048)
    nrows = 2048
    pb = Program()
    pb.nslots = 1 + nrows * M.W
    pb.rows = (1 + np.arange(nrows * M.W, dtype=np.int64)).reshape(nrows, M.W).tolist()
    # inputs spread over the matrix, its last wire included; one generator; the rest stays unset
    cells = sorted(set(rng.sample(range(nrows * M.W), 400)) | {0, nrows * M.W - 1, 1024 * 256 - 1, 1024 * 256})
    pb.in_slots = [1 + c for c in cells]
    out = next(s for s in range(1000, 2000) if s not in set(pb.in_slots))
    pb.emit(M.ARITH, 0, [pb.in_slots[0], pb.in_slots[1], pb.in_slots[2], out], 1, 1)
    ins = np.array([rnd_tuple(rng, len(cells)), [PM1] * len(cells)], np.uint64)
    want, failed, _ = M.run_batch(pb, ins)
    assert not any(failed)
    wslot = np.array(pb.rows, np.uint32)
    wcm = np.ascontiguousarray(wslot.T)
    wires_want = np.where(want[:, wcm] == UNSET, 0, want[:, wcm])
    assert (wires_want != 0).sum() > 0 and (want == UNSET).sum() > nrows * M.W  # set and unset cells both
    pool = pb.in_slots[:150] + [out, 0] + list(range(2, 150))  # written and unset slots
    tabs = pb.tables()
    for npis, form in [(0, N.WFORM_PROOF_256), (1, N.WFORM_LEVEL_ROW), (300, N.WFORM_PROOF_512)]:
        pi_slots = pool[:npis]
        vals, err, wires, pis = run_probe(ctx, form, pb, ins, tabs, wslot_cm=wcm, pi_slots=pi_slots)
        assert not err.any() and (vals == want).all()
        assert wires.shape == (2, M.W, nrows) and (wires == wires_want).all()
        assert pis.shape == (2, npis)
        assert (pis == np.where(want[:, pi_slots] == UNSET, 0, want[:, pi_slots])).all()


# ---- the probe's own refusals --------------------------------------------------------

def good_program():
    pb = Program()
    a, b, c = pb.inputs(3)
    x = pb.slot()
    pb.emit(M.ARITH, 0, [a, b, c, x], 1, 1)                                    # 0
    pb.emit(M.EXT_DIV, 0, pb.inputs(4), pb.slot() | pb.slot() << 32)            # 1
    r0, _ = pb.row(), pb.row()
    pb.emit(M.WIRE_SPLIT, r0, [a, 2])                                          # 2
    pb.emit(M.RANDOM_ACCESS, pb.input_row([0] + list(range(2, 18))), [0])      # 3
    pb.emit(M.ARITH_EXT, pb.input_row(range(6)), [0], 1, 1)                    # 4
    pb.emit(M.MUL_EXT, pb.input_row(range(4)), [0], 1)                         # 5
    pb.emit(M.POSEIDON, pb.input_row(list(range(12)) + [M.PG_SWAP]))           # 6
    return pb


def setf(gens, i, field, value):
    """field of record i: kind, row, s0..s3, k0"""
    word, shift = {"kind": (0, 0), "row": (0, 32), "s0": (1, 0), "s1": (1, 32), "s2": (2, 0), "s3": (2, 32)}.get(
        field, (3, None))
    if shift is None:
        gens[i][word] = value
    else:
        gens[i][word] = (int(gens[i][word]) & ~(0xFFFFFFFF << shift)) | value << shift


def malformed_cases():
    """[(name, mutate(args dict), text)]: one malformed program per validator rule"""
    def rec(i, field, value):
        return lambda d: setf(d["gens"], i, field, value(d) if callable(value) else value)

    def put(key, value):
        return lambda d: d.__setitem__(key, value(d) if callable(value) else value)

    def two_levels(off):
        def f(d):
            d["level_off"] = np.array(off, np.uint32)
            d["level_pos"] = np.array([[6, 1], [7, 0]], np.uint32)
        return f

    def wslot_entry(d):
        d["wslot"][3][5] = d["nslots"]

    def in_slot(v):
        def f(d):
            d["in_slots"] = d["in_slots"].copy()
            d["in_slots"][0] = v(d)
        return f
    ns = lambda d: d["nslots"]  # noqa: E731
    return [
        ("kind", rec(0, "kind", 14), "unknown kind in record 0"),
        ("row", rec(6, "row", lambda d: len(d["wslot"])), "row outside the wire table in record 6"),
        ("wire_split_rows", rec(2, "s1", lambda d: len(d["wslot"]) + 1), "row outside the wire table in record 2"),
        ("slot", rec(0, "s3", ns), "slot outside the slots in record 0"),
        ("slot_multi", rec(0, "s1", lambda d: d["nslots"] | M.MULTI), "slot outside the slots in record 0"),
        ("ext_div_lo", rec(1, "k0", lambda d: d["nslots"] | 1 << 32), "quotient slot outside the slots in record 1"),
        ("ext_div_hi", rec(1, "k0", lambda d: 1 | d["nslots"] << 32), "quotient slot outside the slots in record 1"),
        ("wslot", wslot_entry, "slot outside the slots at wslot entry %d" % (3 * 135 + 5)),
        ("in_slots", in_slot(ns), "slot outside the slots at in_slots entry 0"),
        ("in_slots_flag", in_slot(lambda d: 1 | M.MULTI), "slot outside the slots at in_slots entry 0"),
        ("W", put("wslot", lambda d: np.ascontiguousarray(d["wslot"][:, :134])),
         "W is not 135 for the row-layout record 3"),
        ("limbs", put("limbs", 64), "limbs above 63"),
        ("limbs_W", put("wslot", lambda d: np.ascontiguousarray(d["wslot"][:, :63])), "1 + limbs above W"),
        ("ra_copy", rec(3, "s0", 4), "random-access copy above 3 in record 3"),
        ("ae_op", rec(4, "s0", 10), "arithmetic-extension op above 9 in record 4"),
        ("me_op", rec(5, "s0", 13), "mul-extension op above 12 in record 5"),
        ("level_off_decreases", two_levels([0, 7, 6]), "level_off decreases at level 1"),
        ("level_off_end", put("level_off", np.array([0, 6], np.uint32)), "level_off does not end at the record count"),
        ("run_outside", put("level_pos", np.array([[6, 2]], np.uint32)), "Poseidon run outside level 0"),
        ("run_other_kind", put("level_pos", np.array([[5, 2]], np.uint32)),
         "record that is no Poseidon in the Poseidon run of level 0"),
        ("poseidon_outside_run", put("level_pos", np.array([[7, 0]], np.uint32)),
         "Poseidon record outside the Poseidon run of level 0"),
        ("B", put("in_vals", lambda d: np.zeros((65, d["in_vals"].shape[1]), np.uint64)), "B outside 1..64"),
        ("nslots", put("nslots", (1 << 20) + 1), "nslots outside 1..2^20"),
        ("records", lambda d: d.update(gens=np.zeros((65537, 5), np.uint64), level_off=np.array([0, 65537], np.uint32),
                                       level_pos=np.array([[65537, 0]], np.uint32)), "more than 2^16 records"),
        ("form", put("form", 99), "unknown form"),
    ]


def probe_args(pb, in_vals):
    gens, level_off, level_pos, wslot = pb.tables()
    return dict(form=N.WFORM_PROOF_256, gens=gens, level_off=level_off, level_pos=level_pos, wslot=wslot,
                nslots=pb.nslots, in_slots=np.array(pb.in_slots, np.uint32), in_vals=in_vals, limbs=63)


def test_probe_refuses_malformed_programs(ctx):
    """one malformed program per rule of csrc/witness_program.h: QP_ERR_ARG with
    the rule's text, nothing launched; a good program afterwards still runs"""
    rng = random.Random(4)
    pb = good_program()
    ins = np.array([rnd_tuple(rng, len(pb.in_slots))], np.uint64)
    ins[0][7] %= 16  # the random-access index
    ins[0][-1] &= 1
    for name, mutate, text in malformed_cases():
        d = probe_args(pb, ins)
        mutate(d)
        with pytest.raises(N.QpError) as e:
            N.debug_witness_program(ctx, **d)
        assert e.value.code == 1 and text in str(e.value), (name, str(e.value))
    check(ctx, pb, ins)
