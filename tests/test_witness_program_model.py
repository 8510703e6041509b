"""The witness-program model (witness_program_model.py) held to the gates it
fills, without a GPU: for every kind bound to a gate row, the row the model
produces satisfies every constraint of that gate in the CPU oracle
(ora_gate_eval, with the descriptors of RECURSION_GATES and of the leaf gate
list in test_gpu_seams.py), on random and on edge inputs; the Poseidon row's
output wires are oracle_lib.permute of the (swapped) input; and the builder's
tables and the failure model behave as test_gpu_witness_program.py relies on."""
import random

import numpy as np
import pytest

import witness_program_model as M
from edge_values import CANON_EDGES
from oracle_lib import permute
from test_gpu_seams import RECURSION_GATES
from test_recursion_gates import desc, gate_eval
from witness_program_model import P, Program

PARAMS = {k: p for k, p, _ in RECURSION_GATES}


def values(rng, n, mode):
    if mode == "random":
        return [rng.randrange(P) for _ in range(n)]
    k = rng.randrange(len(CANON_EDGES))
    return [CANON_EDGES[(k + i) % len(CANON_EDGES)] for i in range(n)]


def row_program(kind, rng):
    """(program, gate name, gate constants, rows to check, fix(in_vals)): one full gate row of `kind`"""
    pb = Program()
    k0, k1 = rng.randrange(P), rng.randrange(P)
    fix = None
    if kind == M.POSEIDON:
        r = pb.input_row(list(range(12)) + [M.PG_SWAP])
        pb.emit(kind, r)

        def fix(v):  # the swap wire is a bit
            v[12] = v[12] & 1
        return pb, "poseidon", [0, 0], [r], fix
    if kind == M.BASE_SPLIT:
        r = pb.input_row([0])
        pb.emit(kind, r, [pb.wire(r, 0)])

        def fix(v):  # the gate holds 63 limbs
            v[0] &= (1 << 63) - 1
        return pb, "base_sum", [0, 0], [r], fix
    if kind == M.WIRE_SPLIT:
        x = pb.input()
        r0, r1 = pb.row(), pb.row()
        pb.emit(kind, r0, [x, 2])
        pb.level()
        for r in (r0, r1):
            pb.emit(M.BASE_SPLIT, r, [pb.wire(r, 0)])
        return pb, "base_sum", [0, 0], [r0, r1], None
    if kind == M.RANDOM_ACCESS:
        r = pb.input_row([18 * c + j for c in range(4) for j in [0] + list(range(2, 18))] + [72, 73])
        for c in range(4):
            pb.emit(kind, r, [c])

        def fix(v):  # indices below 16; the extra-constant wires hold the gate's constants
            for c in range(4):
                v[17 * c] %= 16
            v[68], v[69] = k0, k1
        return pb, "random_access", [k0, k1], [r], fix
    if kind in (M.ARITH_EXT, M.MUL_EXT):
        n, w, nin = (10, 8, 6) if kind == M.ARITH_EXT else (13, 6, 4)
        r = pb.input_row([w * i + j for i in range(n) for j in range(nin)])
        for i in range(n):
            pb.emit(kind, r, [i], k0, k1)
        return pb, "arithmetic_extension" if kind == M.ARITH_EXT else "mul_extension", [k0, k1], [r], None
    if kind in (M.REDUCING, M.REDUCING_EXT):
        n = 6 + (43 if kind == M.REDUCING else 64)
        r = pb.input_row(range(2, n))
        pb.emit(kind, r)
        return pb, "reducing" if kind == M.REDUCING else "reducing_extension", [0, 0], [r], None
    if kind == M.POSEIDON_MDS:
        r = pb.input_row(range(24))
        pb.emit(kind, r)
        return pb, "poseidon_mds", [0, 0], [r], None
    if kind == M.COSET_INTERP:
        r = pb.input_row(range(M.CI_EVAL_POINT + 2))
        pb.emit(kind, r)

        def fix(v):
            v[0] = v[0] or 1
        return pb, "coset_interpolation", [0, 0], [r], fix
    raise ValueError(kind)


ROW_KINDS = [M.POSEIDON, M.BASE_SPLIT, M.WIRE_SPLIT, M.RANDOM_ACCESS, M.ARITH_EXT, M.MUL_EXT, M.REDUCING,
             M.REDUCING_EXT, M.POSEIDON_MDS, M.COSET_INTERP]


@pytest.mark.parametrize("mode", ["random", "edge"])
@pytest.mark.parametrize("kind", ROW_KINDS, ids=[M.KIND_NAMES[k] for k in ROW_KINDS])
def test_model_rows_satisfy_their_gates(kind, mode):
    rng = random.Random(100 * kind + len(mode))
    pb, gate, consts, rows, fix = row_program(kind, rng)
    d = desc(gate, PARAMS[gate])
    for _ in range(3):
        v = values(rng, len(pb.in_slots), mode)
        if fix:
            fix(v)
        vals, failed, _ = M.run(pb, v)
        assert not failed
        wires = M.expand(pb, vals)
        for r in rows:
            out = gate_eval(d, [col[r] for col in wires], consts)
            assert len(out) > 0 and out == [0] * len(out), (M.KIND_NAMES[kind], r)


@pytest.mark.parametrize("swap", [0, 1])
def test_poseidon_row_output_is_the_permutation(swap):
    rng = random.Random(7 + swap)
    for state in ([rng.randrange(P) for _ in range(12)], [P - 1] * 12, [0] * 12, list(CANON_EDGES[:12])):
        w = M.poseidon_row(state, swap)
        s = list(state)
        if swap:
            s[0:4], s[4:8] = s[4:8], s[0:4]
        assert [w[M.PG_OUT + i] for i in range(12)] == [int(x) for x in permute(s)]
        assert sorted(w) == list(range(12, 24)) + list(range(25, 135))


def test_ext_div_and_equality_definitions():
    rng = random.Random(3)
    for den in [(0, 5), (7, 0), (P - 1, P - 1), (rng.randrange(P), rng.randrange(P))]:
        num = (rng.randrange(P), P - 1)
        assert M.emul(M.ext_div(num, den), den) == num


def test_builder_tables():
    pb = Program()
    a, b, c = pb.inputs(3)
    o1, o2 = pb.slot(), pb.slot()
    pb.emit(M.ARITH, 0, [a, b, c, o1], 1, 1)
    r = pb.input_row(list(range(12)) + [M.PG_SWAP])
    pb.emit(M.POSEIDON, r)
    pb.level()
    pb.level()
    pb.emit(M.ARITH, 0, [a, b, c, o1], 1, 1)  # o1 has two writers
    pb.level()
    pb.emit(M.ARITH, 0, [a, o1, c, o2], 2, 3)
    gens, level_off, level_pos, wslot = pb.tables()
    assert gens.shape == (4, 5) and list(level_off) == [0, 2, 2, 3, 4]
    assert level_pos.tolist() == [[1, 1], [2, 0], [3, 0], [4, 0]]
    assert wslot.shape == (1, 135) and not (wslot & M.MULTI).any()
    assert int(gens[0][2]) >> 32 == o1 | M.MULTI and int(gens[3][1]) >> 32 == o1 | M.MULTI
    assert int(gens[3][2]) >> 32 == o2
    assert int(gens[1][0]) == M.POSEIDON | r << 32
    vals, failed, first = M.run(pb, [2, 3, 4] + [0] * 13)
    assert not failed and vals[o1] == 10 and vals[o2] == (2 * 2 * 10 + 3 * 4)


def test_failure_model():
    pb = Program()
    a, b = pb.inputs(2)
    x, y, z, unset = pb.slots(4)
    pb.emit(M.ARITH, 0, [a, a, a, x], 1, 0)        # 0: x = a^2
    pb.level()
    pb.emit(M.ARITH, 0, [a, b, a, x], 1, 0)        # 1: x = a b: a conflict unless a == b
    pb.emit(M.ARITH, 0, [unset, a, a, y], 1, 0)    # 2: reads a slot nobody writes
    pb.level()
    pb.emit(M.ARITH, 0, [y, a, a, z], 1, 0)        # 3: downstream of 2
    _, failed, first = M.run(pb, [5, 5])
    assert failed == {2, 3} and first == [2]
    _, failed, first = M.run(pb, [5, 6])
    assert failed == {1, 2, 3} and first == [1, 2]


def test_expand_reads_unset_as_zero():
    pb = Program()
    r = pb.input_row([3])
    vals, _, _ = M.run(pb, [9])
    wires = M.expand(pb, vals)
    assert wires[3][r] == 9 and sum(map(sum, wires)) == 9
    assert np.array(wires).shape == (135, 1)
