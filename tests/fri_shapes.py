"""FRI shapes beyond the fixtures' arity-16 reductions, for the native verifier's
tests (test_verifier_fri_shapes.py on the host path, test_gpu_verifier.py on the
device).  The oracle prover takes the FRI shape from the common data it is
handed and the transcript takes the circuit digest as data, so one witness of
the voting circuit (2^8 rows, rate_bits 3, N = 2^11) proves under any patched
shape; ora_verify is the checker.  Test infrastructure, nothing committed as a
fixture.
"""
import ctypes
import functools
import random
import struct

import numpy as np

import verifier_cases as vc
from oracle_lib import U64P, lib as olib

FRI_CONFIGS = (50, 95)  # CommonCircuitData carries FriConfig twice: in the circuit config and in the FRI parameters
ARITY_AT = 140          # u64 count, then that many u64 arity_bits
POW_BITS = 8            # grinding stays trivial; a tampered final polynomial still fails PoW (255 / 256)

# (arity_bits per layer, cap height, query rounds); log_n = 8 and rate_bits = 3 throughout.
# The smallest shapes that reach each branch of the query rounds:
SHAPES = (
    ((), 4, 28),            # no layers: 256-coefficient final polynomial, largest pp_stride, initial value against it
    ((1,), 4, 28),          # arity 2: layer leaf of width 4 (hash_or_noop in the query rounds), 2-point interpolation
    ((2, 3), 4, 28),        # mixed arities 4 and 8, rev_bits at widths 2 and 3
    ((3, 2, 1), 4, 28),     # descending mix, three layers
    ((5,), 4, 28),          # arity 32
    ((6,), 4, 28),          # arity 64, the bound
    ((6, 1), 4, 28),        # arity 64 then 2; the last layer's tree is all cap (no siblings)
    ((1,) * 7, 4, 28),      # 11 path classes; last layer all cap
    ((1,) * 8, 0, 28),      # MAX_LAYERS and MAX_CLASSES, cap height 0, final polynomial of one coefficient
    ((1,) * 8, 3, 1),       # one query: one lane per class
    ((4, 3), 4, 63),        # odd nq near the bound: odd lane counts, index-array padding
    ((2, 2, 2, 2), 2, 5),   # small odd nq, low cap
    ((4, 4), 3, 64),        # nq at its bound, fully reduced
)


def shape_id(shape):
    arity, cap_h, nq = shape
    return "a%s-c%d-q%d" % ("".join(map(str, arity)) or "none", cap_h, nq)


def patch_common(cb, arity, cap_h=None, nq=None, pow_bits=None):
    """CommonCircuitData bytes cb with another FRI shape: both FriConfig copies
    (rate_bits u64 +0, cap_height u64 +8, num_query_rounds u64 +16, pow bits u32
    +24) and the arity list, the tail respliced after it."""
    arity = list(arity)
    was = vc.parse_common(cb)
    b = bytearray(cb)
    for base in FRI_CONFIGS:
        if cap_h is not None:
            struct.pack_into("<Q", b, base + 8, cap_h)
        if nq is not None:
            struct.pack_into("<Q", b, base + 16, nq)
        if pow_bits is not None:
            struct.pack_into("<I", b, base + 24, pow_bits)
    tail = ARITY_AT + 8 + 8 * len(was["arity"])
    out = bytes(b[:ARITY_AT]) + struct.pack("<Q", len(arity)) + b"".join(struct.pack("<Q", a) for a in arity) + \
        bytes(b[tail:])
    now = vc.parse_common(out)
    want = dict(was, arity=arity, cap_h=was["cap_h"] if cap_h is None else cap_h, nq=was["nq"] if nq is None else nq)
    assert now == want, (now, want)
    first, second = (struct.unpack_from("<QQQI", out, base) for base in FRI_CONFIGS)
    assert first == second == (was["rate_bits"], want["cap_h"], want["nq"],
                               struct.unpack_from("<I", cb, 50 + 24)[0] if pow_bits is None else pow_bits)
    return out


@functools.lru_cache(maxsize=None)
def _voting():
    """(circuit, constants||sigmas, wires, public inputs) of one voting witness."""
    from qp_wormhole import Circuit
    from qp_wormhole.synthetic import synthetic_vote_inputs
    circ = Circuit.voting()
    w = circ.commit(synthetic_vote_inputs(2, 5))
    return (circ, circ.constants_sigmas(), np.ascontiguousarray(w.wires(), np.uint64),
            np.ascontiguousarray(w.public_inputs(), np.uint64))


def voting_common():
    return _voting()[0].common_data()


@functools.lru_cache(maxsize=None)
def oracle_case(shape):
    """(verifier_only, common, proof): the oracle's proof of the voting witness under `shape`."""
    arity, cap_h, nq = shape
    circ, cs, wires, pis = _voting()
    cb = patch_common(circ.common_data(), arity, cap_h, nq, POW_BITS)
    L = olib()
    L.ora_prove.argtypes = [ctypes.c_char_p, ctypes.c_size_t, U64P, U64P, U64P, ctypes.c_size_t, ctypes.c_char_p,
                            ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), U64P, U64P]
    room = 1 << 22
    out = ctypes.create_string_buffer(room)
    ln = ctypes.c_size_t()
    cap = np.zeros(4 << 4, np.uint64)
    dig = np.zeros(4, np.uint64)
    assert cap_h <= 4
    assert L.ora_prove(cb, len(cb), cs, wires, pis, len(pis), out, room, ctypes.byref(ln), cap, dig) == 0
    vo = struct.pack("<Q", cap_h) + cap[:4 << cap_h].tobytes() + dig.tobytes()
    pf = out.raw[:ln.value]
    assert vc.ora(vo + cb, pf) == 0
    return vo, cb, pf


@functools.lru_cache(maxsize=None)
def tamper_cases(shape):
    """[(label, proof, oracle rc)] over verifier_cases.tamper_set of oracle_case(shape)."""
    vo, cb, pf = oracle_case(shape)
    vd = vo + cb
    return tuple((lab, p, vc.ora(vd, p)) for lab, p in vc.tamper_set(vd, cb, pf))


def status_floor(shape):
    """The statuses the tamper set of a shape must produce, so that no test passes by rejecting
    everything at one stage.  6 and 7 need a layer.  8 (final polynomial) is out of a byte
    tamper's reach: the final polynomial is observed before PoW and the query indices."""
    return {0, 3, 4, 5, 6, 7, 9} if shape[0] else {0, 3, 4, 5, 9}


def chunk_pick(shape):
    """A fixed seeded pick of 7 proofs from the tamper pool of `shape`, run as chunks of 3, 3, 1:
    valid at 0, 4, 5, 6 and tampered at 1, 2, 3, so that each chunk position holds a valid proof
    in one chunk and a tampered one in another (a slot reading its neighbour's arrays shows), and
    the one-proof chunk's only slot is a valid proof whose every lane counts.  Of the tampered
    three, two fail in the query rounds (5..7) and one before them (its slot is cleared)."""
    cases = tamper_cases(shape)
    rng = random.Random(7)
    valid = [True, False, False, False, True, True, True]
    in_rounds = [p for _, p, rc in cases if 5 <= rc <= 7]
    before = [p for _, p, rc in cases if rc and not 5 <= rc <= 7]
    tampered = rng.sample(in_rounds, 2) + rng.sample(before, 1)
    rng.shuffle(tampered)
    return [cases[0][1] if ok else tampered.pop() for ok in valid], valid
