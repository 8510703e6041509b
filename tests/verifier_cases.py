"""Accept-and-tamper cases for the native verifier's tests (test_verifier.py on
the host path, test_gpu_verifier.py on the device): the reference's three
proofs, each with one bit flipped per region of the serialized proof, offsets
computed from the layout in the common data (as
current_circuit_vd.parse_queries walks it).  The oracle is the checker: every
case carries ora_verify's return code.  Test infrastructure.
"""
import functools
import struct

import numpy as np

from oracle_lib import P, golden, lib as olib


def parse_common(cb):
    """The fields of CommonCircuitData the proof layout depends on."""
    u64 = lambda o: struct.unpack_from("<Q", cb, o)[0]  # noqa: E731
    d = {"num_wires": u64(0), "num_routed": u64(8), "nc": u64(32), "rate_bits": u64(50), "cap_h": u64(58), "nq": u64(66)}
    o = 140
    na = u64(o)
    d["arity"] = [u64(o + 8 + 8 * i) for i in range(na)]
    o += 8 + 8 * na
    d["degree_bits"] = u64(o)
    d["hiding"] = cb[o + 8]
    o += 9
    o += 8 + 8 * u64(o)           # selector indices
    o += 8 + 16 * u64(o)          # selector groups
    d["qdf"], d["num_constants"] = u64(o), u64(o + 16)
    o += 32
    o += 8 + 8 * u64(o)           # k_is
    d["npp"] = u64(o)
    return d


class Layout:
    """Byte offsets inside a proof of the circuit with common data cb."""

    def __init__(self, cb):
        d = parse_common(cb)
        self.d = d
        nc, salt = d["nc"], 4 if d["hiding"] else 0
        self.cap_bytes = 32 << d["cap_h"]
        self.unsalted = [d["num_constants"] + d["num_routed"], d["num_wires"], nc * (1 + d["npp"]), nc * d["qdf"]]
        self.widths = [self.unsalted[0]] + [w + salt for w in self.unsalted[1:]]
        self.log_N = d["degree_bits"] + d["rate_bits"]
        self.init_sibs = self.log_N - d["cap_h"]
        self.openings = 3 * self.cap_bytes
        # constants||sigmas, wires, zs, zs_next, partial products, quotient
        self.open_at = {"constants": 0, "wires": self.unsalted[0], "quotient": sum(self.unsalted) + nc - self.unsalted[3]}
        nopen = sum(self.unsalted) + nc
        self.layer_caps = self.openings + 16 * nopen
        self.queries = self.layer_caps + len(d["arity"]) * self.cap_bytes
        lg, self.layers = self.log_N, []
        for a in d["arity"]:
            lg -= a
            self.layers.append((a, lg - d["cap_h"]))
        self.query_bytes = sum(8 * w + 1 + 32 * self.init_sibs for w in self.widths) + \
            sum((16 << a) + 1 + 32 * s for a, s in self.layers)
        self.final_poly = self.queries + d["nq"] * self.query_bytes
        self.final_len = 1 << (d["degree_bits"] - sum(d["arity"]))
        self.pow = self.final_poly + 16 * self.final_len
        self.npis = self.pow + 8

    def tree(self, q, o):
        """(leaf offset, sibling-count byte offset) of initial tree o in query q."""
        off = self.queries + q * self.query_bytes
        for w in self.widths[:o]:
            off += 8 * w + 1 + 32 * self.init_sibs
        return off, off + 8 * self.widths[o]

    def layer(self, q, l):
        """(evals offset, sibling-count byte offset) of FRI layer l in query q."""
        off = self.tree(q, 3)[1] + 1 + 32 * self.init_sibs
        for a, s in self.layers[:l]:
            off += (16 << a) + 1 + 32 * s
        return off, off + (16 << self.layers[l][0])


def query_indices(vd, pf, lay):
    """The transcript's query indices (ora_challenges)."""
    out = np.zeros(256, np.uint64)
    n = olib().ora_challenges(vd, len(vd), pf, len(pf), out)
    assert n > 0
    return [int(x) for x in out[n - lay.d["nq"]:n]]


def flip(pf, off, bit=0):
    b = bytearray(pf)
    b[off] ^= 1 << bit
    return bytes(b)


def tamper_set(vd, cb, pf):
    """[(label, proof bytes)]: the proof itself first, then the tampered variants.
    Valid for any FRI shape the verifier accepts: the query picks are clamped to
    nq and deduplicated (nq = 1 has one), and a layer whose tree is all cap has
    no sibling to change, so another element of its leaf is changed instead."""
    lay = Layout(cb)
    nq = lay.d["nq"]
    qidx = query_indices(vd, pf, lay)
    cases = [("intact", pf), ("wires cap", flip(pf, 8 * 5))]
    for what, k in (("constants", 3), ("wires", 5), ("quotient", 1)):
        cases.append((f"{what} opening", flip(pf, lay.openings + 16 * (lay.open_at[what] + k))))
    cases.append(("public input", flip(pf, len(pf) - 100)))
    cases.append(("pow witness", flip(pf, lay.pow + 1)))
    for q in dict.fromkeys((0, nq // 2, nq - 1)):
        for o in range(4):
            leaf, nsib = lay.tree(q, o)
            cases.append((f"q{q} tree{o} leaf", flip(pf, leaf + 8 * (lay.widths[o] // 2))))
            cases.append((f"q{q} tree{o} sibling", flip(pf, nsib + 1 + 32 * (lay.init_sibs // 2) + 9)))
    q, shift = nq // 2, 0
    for l, (a, s) in enumerate(lay.layers):
        ev, nsib = lay.layer(q, l)
        within = (qidx[q] >> shift) & ((1 << a) - 1)
        shift += a
        cases.append((f"layer{l} queried element", flip(pf, ev + 16 * within + 2)))
        cases.append((f"layer{l} other element", flip(pf, ev + 16 * ((within + 3) % (1 << a)) + 10)))
        if s:
            cases.append((f"layer{l} sibling", flip(pf, nsib + 1 + 32 * (s - 1) + 17)))
        else:
            cases.append((f"layer{l} leaf, no sibling", flip(pf, ev + 16 * ((within + 1) % (1 << a)) + 1)))
    cases.append(("final poly", flip(pf, lay.final_poly + 16 * (lay.final_len // 2))))
    cases.append(("truncated", pf[:-1]))
    cases.append(("extra byte", pf + b"\0"))
    cases.append(("sibling count", flip(pf, lay.tree(min(1, nq - 1), 2)[1], 1)))
    at = lay.tree(min(2, nq - 1), 1)[0] + 8 * 7
    cases.append(("element = p", pf[:at] + struct.pack("<Q", P) + pf[at + 8:]))
    return cases


def ora(vd, pf):
    return olib().ora_verify(vd, len(vd), pf, len(pf))


def expect(rc):
    """The native verifier's status for the oracle's return code."""
    return rc if rc <= 8 else 9


@functools.lru_cache(maxsize=None)
def current_vd():
    """(verifier-only, common) of the current degree-13 circuit."""
    from current_circuit_vd import current_circuit_verifier_data
    from test_oracle_golden import current_common_bytes
    cb = current_common_bytes()
    vd = current_circuit_verifier_data(cb)[0]
    return vd[:len(vd) - len(cb)], cb


@functools.lru_cache(maxsize=None)
def bench_vd():
    """(verifier-only, common) of the reference's bench fixture (degree 14, salted)."""
    cb, vb = golden("common.bin"), golden("verifier.bin")
    assert vb.endswith(cb)
    return vb[:len(vb) - len(cb)], cb


@functools.lru_cache(maxsize=None)
def reference_cases():
    """{fixture name: (verifier-only, common, [(label, proof, oracle rc)])} for the three proofs."""
    out = {}
    for name, (vo, cb) in (("proof.bin", bench_vd()), ("dummy_proof.bin", current_vd()),
                           ("dummy_proof_zk.bin", current_vd())):
        vd = vo + cb
        out[name] = (vo, cb, [(lab, pf, ora(vd, pf)) for lab, pf in tamper_set(vd, cb, golden(name))])
    return out
