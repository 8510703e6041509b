"""The native verifier on its host path (device=None, no GPU): accepts the
reference's proofs, and gives the oracle's verdict, code for code, on every
tampered variant.  The oracle (oracle/verifier.c) is the checker only; the
verifier under test links nothing of it."""
import ctypes
import struct

import pytest

import verifier_cases as vc
from agg_oracle_backend import oracle_backend
from oracle_lib import golden

NAMES = ("proof.bin", "dummy_proof.bin", "dummy_proof_zk.bin")


def host_verifier(vo, cb, max_batch=64):
    from qp_wormhole import WormholeVerifier
    return WormholeVerifier.new_from_bytes(vo, cb, device=None, max_batch=max_batch)


@pytest.fixture(scope="module")
def verifiers():
    vs = {"bench": host_verifier(*vc.bench_vd()), "current": host_verifier(*vc.current_vd())}
    yield lambda name: vs["bench" if name == "proof.bin" else "current"]
    for v in vs.values():
        v.close()


@pytest.mark.parametrize("name", NAMES)
def test_reference_proofs_verify(verifiers, name):
    vo, cb, cases = vc.reference_cases()[name]
    label, pf, rc = cases[0]
    assert label == "intact" and rc == 0
    assert verifiers(name).verify_batch([pf]) == [0]
    verifiers(name).verify(pf)


def test_new_from_files_bench_shape(tmp_path):
    """The reference's bench (verifier/benches/verifier.rs): new_from_files on
    bench-data's verifier.bin / common.bin, then verify(proof.bin); verifier.bin
    carries the common data after the verifier-only part."""
    import os
    from oracle_lib import GOLDEN
    from qp_wormhole import WormholeVerifier
    v = WormholeVerifier.new_from_files(os.path.join(GOLDEN, "verifier.bin"), os.path.join(GOLDEN, "common.bin"),
                                        device=None)
    v.verify(golden("proof.bin"))
    with pytest.raises(ValueError, match="proof verification failed: vanishing/quotient identity"):
        v.verify(vc.flip(golden("proof.bin"), 40))
    v.close()


@pytest.mark.parametrize("name", NAMES)
def test_verdicts_equal_the_oracles(verifiers, name):
    """One bit flipped per region (a cap, three openings, a public input, the
    PoW witness, leaf and sibling of each initial tree in the first, a middle
    and the last query, per FRI layer the queried coset element, another one
    and a sibling, a final-polynomial coefficient), plus a truncated proof, an
    extra byte, a changed sibling-count byte and an element set to p: the status
    equals the oracle's code on every case, and the oracle's codes cover 3, 4,
    5, 6, 7 and malformed.  Codes 2 (zeta in the subgroup) and 8 (final
    polynomial) cannot be reached by tampering without re-grinding the
    transcript: they are covered on the accept side only."""
    vo, cb, cases = vc.reference_cases()[name]
    got = verifiers(name).verify_batch([pf for _, pf, _ in cases])
    bad = [(lab, st, rc) for (lab, _, rc), st in zip(cases, got) if st != vc.expect(rc)]
    assert not bad, bad
    codes = {vc.expect(rc) for _, _, rc in cases}
    assert {0, 3, 4, 5, 6, 7, 9} <= codes, codes


@pytest.fixture(scope="module")
def level1():
    import qp_wormhole
    vo, cb = vc.current_vd()
    return qp_wormhole.aggregate_chunk([golden("dummy_proof.bin"), golden("dummy_proof_zk.bin")], cb, vo,
                                       backend=oracle_backend)


def test_aggregation_proof(level1):
    """A level-1 aggregation proof: the seven recursion gates' constraints at zeta."""
    cd = level1.circuit_data
    pf = level1.proof.to_bytes()
    vd = cd.verifier_data()
    lay = vc.Layout(cd.common)
    bad = vc.flip(pf, lay.openings + 16 * (lay.open_at["wires"] + 50) + 3)
    assert vc.ora(vd, pf) == 0 and vc.ora(vd, bad) == 3
    v = host_verifier(cd.verifier_only, cd.common)
    assert v.verify_batch([pf, bad]) == [0, 3]
    v.close()


def test_wrong_verifier_data(verifiers):
    vo, cb = vc.current_vd()
    pf = golden("dummy_proof.bin")
    for off in (8 + 5 * 32, len(vo) - 8):  # a cap element, a digest element
        bad = vc.flip(vo, off)
        rc = vc.ora(bad + cb, pf)
        v = host_verifier(bad, cb)
        st = v.verify_batch([pf])[0]
        v.close()
        assert st == vc.expect(rc) and st != 0
    # another circuit's data: the bench circuit's cap and digest with this circuit's common data
    other = vc.bench_vd()[0]
    rc = vc.ora(other + cb, pf)
    v = host_verifier(other, cb)
    assert v.verify_batch([pf])[0] == vc.expect(rc) != 0
    v.close()


def _new(vo, cb):
    from qp_wormhole import lib
    h = ctypes.c_void_p()
    rc = lib().qp_verifier_new(None, vo, len(vo), cb, len(cb), 4, ctypes.byref(h))
    msg = lib().qp_verifier_last_error(h).decode() if h else ""
    # a handle that only carries the reason verifies nothing
    if rc:
        st = (ctypes.c_uint32 * 1)()
        assert lib().qp_verifier_verify(h, None, None, 1, st) == 4
    lib().qp_verifier_free(h)
    return rc, msg


def test_constructor_errors(tmp_path):
    from qp_wormhole import QpError, WormholeVerifier
    vo, cb = vc.current_vd()
    assert _new(vo, cb) == (0, "")
    rc, msg = _new(vo, cb[:-9])
    assert rc == 6 and "malformed CommonCircuitData" in msg
    assert struct.unpack_from("<I", cb, len(cb) - 4)[0] == 11  # the last gate: Poseidon, no parameters
    rc, msg = _new(vo, cb[:-4] + struct.pack("<I", 5))    # a lookup gate's tag
    assert rc == 6 and "unsupported gate" in msg
    # a gate parameter whose products would wrap 64 bits (BaseSum's limb count, Arithmetic's op count)
    for tag in (2, 0):
        at = [i for i in range(len(cb) - 12, 180, -1) if struct.unpack_from("<I", cb, i)[0] == tag
              and 0 < struct.unpack_from("<Q", cb, i + 4)[0] <= 64]
        assert at, tag
        for huge in (2**64 - 1, 2**63, 2**62, 136):
            rc, msg = _new(vo, cb[:at[0] + 4] + struct.pack("<Q", huge) + cb[at[0] + 12:])
            assert rc == 6 and "gate" in msg, (tag, huge, rc, msg)
    rc, msg = _new(vo + b"\0", cb)
    assert rc == 6 and "verifier data" in msg
    rc, msg = _new(struct.pack("<Q", 3) + vo[8:], cb)
    assert rc == 6 and "cap height" in msg
    with pytest.raises(ValueError, match="^Failed to deserialize common circuit data from bytes$"):
        WormholeVerifier.new_from_bytes(vo, cb[:-9], device=None)
    with pytest.raises(ValueError, match="^Failed to deserialize verifier data from bytes$"):
        WormholeVerifier.new_from_bytes(vo[:-1], cb, device=None)
    vp, cp = tmp_path / "verifier.bin", tmp_path / "common.bin"
    vp.write_bytes(vo)
    cp.write_bytes(cb[:-9])
    with pytest.raises(ValueError, match="Failed to deserialize common circuit data from .*common.bin"):
        WormholeVerifier.new_from_files(vp, cp, device=None)
    vp.write_bytes(vo[:100])
    with pytest.raises(ValueError, match="Failed to deserialize verifier data from .*verifier.bin"):
        WormholeVerifier.new_from_files(vp, cp, device=None)
    with pytest.raises(ValueError, match="unknown circuit config"):
        WormholeVerifier("fast_config", device=None)
    assert QpError  # the non-format failures stay QpError


def test_batch_semantics(verifiers):
    v = verifiers("dummy_proof.bin")
    assert v.verify_batch([]) == []
    cases = vc.reference_cases()
    a, z = golden("dummy_proof.bin"), golden("dummy_proof_zk.bin")
    bad1 = cases["dummy_proof.bin"][2][5][1]      # a tampered opening
    bad3 = cases["dummy_proof_zk.bin"][2][10][1]  # a tampered query
    batch = [a, bad1, z, bad3, a]
    alone = [v.verify_batch([p])[0] for p in batch]
    assert alone[0] == alone[2] == alone[4] == 0 and alone[1] and alone[3]
    assert v.verify_batch(batch) == alone
    small = host_verifier(*vc.current_vd(), max_batch=2)  # chunks of 2, 2, 1
    assert small.verify_batch(batch) == alone
    small.close()
