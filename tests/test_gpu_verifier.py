"""The native verifier's device path: the Merkle path kernel at its smallest
shapes (qp_merkle_verify), the query-round kernels over batches of the
reference's proofs and their tampered variants (statuses equal to the host
path's and the oracle's), and proofs from this backend's own provers."""
import os

import numpy as np
import pytest

import fri_shapes as fs
import verifier_cases as vc
from current_circuit_vd import cap_entry
from oracle_lib import GOLDEN, P, golden, lib as olib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def device_verifier(vo, cb, max_batch=64):
    from qp_wormhole import WormholeVerifier
    return WormholeVerifier.new_from_bytes(vo, cb, device=0, max_batch=max_batch)


@pytest.fixture(scope="module")
def current():
    v = device_verifier(*vc.current_vd())
    yield v
    v.close()


def oracle_path_ok(leaf, idx, sibs, cap):
    entry, root = cap_entry(leaf, sibs.reshape(-1), int(idx))
    return entry < len(cap) and tuple(int(x) for x in cap[entry]) == root


# widths: hash_or_noop's boundary (<= 4 padded, 5 hashed), the sponge rate (8 | 9), the wires leaf;
# nsib: the leaf is the cap entry, one level, several levels
@pytest.mark.parametrize("nsib", [0, 1, 5])
@pytest.mark.parametrize("width", [1, 4, 5, 8, 9, 135])
def test_merkle_verify_small_shapes(ctx, width, nsib):
    import qp_wormhole
    rng = np.random.default_rng(100 * width + nsib)
    log_n, rate_bits, cap_h = (2, 1, 3 - nsib) if nsib < 2 else (5, 1, 1)
    N = 1 << (log_n + rate_bits)
    vals = rng.integers(0, P, size=(width, 1 << log_n), dtype=np.uint64)
    batch = qp_wormhole.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h)
    all_leaves = np.ascontiguousarray(batch.lde().T)
    # the tree itself against the oracle's
    want_cap = np.zeros((1 << cap_h, 4), np.uint64)
    every = np.arange(N, dtype=np.uint64)
    want_sibs = np.zeros((N, nsib, 4), np.uint64)
    assert olib().ora_merkle(all_leaves, log_n + rate_bits, width, cap_h, want_cap, every, N, want_sibs) == 0
    assert (batch.cap == want_cap).all()
    for n in (1, 63, 65):
        idx = rng.integers(0, N, size=n).astype(np.uint32)
        leaves, sibs = batch.open(idx)
        assert (leaves == all_leaves[idx]).all() and (sibs == want_sibs[idx]).all()
        assert qp_wormhole.merkle_verify(ctx, leaves, idx, sibs, batch.cap).all()
        changes = [("leaf", n // 2), ("index", n - 1)] + ([("sibling", n // 3)] if nsib else [])
        for what, at in changes:
            lv, ix, sb = leaves.copy(), idx.copy(), sibs.copy()
            if what == "leaf":
                lv[at, width - 1] ^= np.uint64(2)
            elif what == "index":
                ix[at] ^= 1
            else:
                sb[at, nsib - 1, 2] ^= np.uint64(1)
            got = qp_wormhole.merkle_verify(ctx, lv, ix, sb, batch.cap)
            want = [oracle_path_ok(lv[i], ix[i], sb[i], batch.cap) for i in range(n)]
            assert list(got) == want and [i for i in range(n) if not got[i]] == [at], (n, what)
    # an index past the tree has no cap entry
    leaves, sibs = batch.open(np.zeros(1, np.uint32))
    assert not qp_wormhole.merkle_verify(ctx, leaves, np.array([N], np.uint32), sibs, batch.cap)[0]
    batch.free()


def test_merkle_verify_deepest_path(ctx):
    """nsib = 32 with cap_height = 0, the largest shape qp_merkle_verify accepts: one lane, a
    path of 32 siblings from an index with its high bits set (the tree need not exist: the cap
    is the root the oracle's climb gives).  The cap entry is index >> 32 = 0 whatever the
    index, so the lane must read cap[0], and a changed index bit at any height must fail."""
    import qp_wormhole
    rng = np.random.default_rng(32)
    leaf = rng.integers(0, P, size=(1, 9), dtype=np.uint64)
    sibs = rng.integers(0, P, size=(1, 32, 4), dtype=np.uint64)
    for index in (0xFFFFFFF5, 0x80000000, 3):
        idx = np.array([index], np.uint32)
        entry, root = cap_entry(leaf[0], sibs.reshape(-1), index)
        assert entry == 0
        cap = np.array([root], np.uint64)
        assert qp_wormhole.merkle_verify(ctx, leaf, idx, sibs, cap)[0]
        for bit in (0, 31):
            assert not qp_wormhole.merkle_verify(ctx, leaf, idx ^ np.uint32(1 << bit), sibs, cap)[0]
    # one more sibling, or a cap above such a path, is outside the accepted shapes
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        qp_wormhole.merkle_verify(ctx, leaf, idx, rng.integers(0, P, size=(1, 33, 4), dtype=np.uint64), cap)
    with pytest.raises(qp_wormhole.QpError, match="QP_ERR_ARG"):
        qp_wormhole.merkle_verify(ctx, leaf, idx, sibs, np.zeros((2, 4), np.uint64))


def test_device_equals_host_equals_oracle(current):
    """The whole accept-and-tamper set of test_verifier.py, one batch per
    circuit through a device verifier."""
    from qp_wormhole import WormholeVerifier
    cases = vc.reference_cases()
    bench = device_verifier(*vc.bench_vd())
    for names, dev in ((("proof.bin",), bench), (("dummy_proof.bin", "dummy_proof_zk.bin"), current)):
        batch = [c for n in names for c in cases[n][2]]
        host = WormholeVerifier.new_from_bytes(dev.verifier_only, dev.common, device=None)
        proofs = [pf for _, pf, _ in batch]
        got, on_host = dev.verify_batch(proofs), host.verify_batch(proofs)
        host.close()
        want = [vc.expect(rc) for _, _, rc in batch]
        assert got == on_host == want, [(lab, g, h, w) for (lab, _, _), g, h, w in zip(batch, got, on_host, want)
                                        if not g == h == w]
        assert {0, 3, 4, 5, 6, 7, 9} <= set(got)
    bench.close()


@pytest.mark.parametrize("shape", fs.SHAPES, ids=fs.shape_id)
def test_fri_shapes_device_equals_host_equals_oracle(shape):
    """k_verify_paths / k_verify_fri at the FRI shapes beyond the fixtures' arity-16 reductions
    (fri_shapes.SHAPES: arities 2..64 and mixes, 0 and 8 layers, 12 path classes, all-cap layer
    trees, width-4 layer leaves, cap height 0, 1 / odd / 64 queries): the oracle's proof of the
    voting circuit under the shape and its whole tamper set in one chunk.  The statuses must
    cover every stage a byte tamper reaches (fri_shapes.status_floor; 8, the final polynomial,
    is out of reach: it is observed before PoW and the query indices)."""
    from qp_wormhole import WormholeVerifier
    vo, cb, _ = fs.oracle_case(shape)
    batch = fs.tamper_cases(shape)
    proofs = [pf for _, pf, _ in batch]
    dev = device_verifier(vo, cb, max_batch=len(proofs))
    host = WormholeVerifier.new_from_bytes(vo, cb, device=None, max_batch=len(proofs))
    got, on_host = dev.verify_batch(proofs), host.verify_batch(proofs)
    dev.close()
    host.close()
    want = [vc.expect(rc) for _, _, rc in batch]
    assert got == on_host == want, [(lab, g, h, w) for (lab, _, _), g, h, w in zip(batch, got, on_host, want)
                                    if not g == h == w]
    assert fs.status_floor(shape) <= set(got), sorted(set(got))


@pytest.mark.parametrize("shape", [fs.SHAPES[10], fs.SHAPES[11]], ids=fs.shape_id)
def test_fri_shapes_odd_lane_chunks(shape):
    """[4,3] / 63 queries and [2,2,2,2] / 5 queries through a device verifier of max_batch = 3:
    7 proofs run as chunks of 3, 3, 1, each with an odd lane count (the u32 index arrays end in
    a padded word), and 3 * 63 lanes * 6 classes cross several 256-lane blocks and class
    boundaries inside a block.  Statuses equal each proof verified alone and the oracle's; the
    pick (fri_shapes.chunk_pick) puts a valid and a tampered proof at every chunk
    position, so a slot reading its neighbour's arrays shows."""
    vo, cb, _ = fs.oracle_case(shape)
    proofs, valid = fs.chunk_pick(shape)
    want = [vc.expect(vc.ora(vo + cb, p)) for p in proofs]
    assert [w == 0 for w in want] == valid
    one = device_verifier(vo, cb, max_batch=1)
    alone = [one.verify_batch([p])[0] for p in proofs]
    one.close()
    dev = device_verifier(vo, cb, max_batch=3)
    assert dev.max_batch == 3
    got = dev.verify_batch(proofs)
    dev.close()
    assert got == alone == want, (got, alone, want)


@pytest.mark.parametrize("n", [1, 2, 65, 130])
def test_ragged_batches_are_independent(current, n):
    """max_batch = 64, so 65 and 130 run in chunks; a fixed seeded pattern of the
    two dummy proofs and their tampered variants."""
    cases = vc.reference_cases()
    pool = [pf for name in ("dummy_proof.bin", "dummy_proof_zk.bin") for _, pf, _ in cases[name][2]]
    rng = np.random.default_rng(7)
    pick = [int(k) for k in rng.integers(0, len(pool), size=n)]
    pick = [0 if rng.random() < 0.4 else k for k in pick]  # a good share of valid proofs
    alone = {k: current.verify_batch([pool[k]])[0] for k in sorted(set(pick))}
    assert current.max_batch == 64
    assert current.verify_batch([pool[k] for k in pick]) == [alone[k] for k in pick]


@pytest.mark.parametrize("config", ["standard_recursion_config", "standard_recursion_zk_config"])
def test_wormhole_prover_proofs(config):
    import qp_wormhole
    from qp_wormhole.synthetic import synthetic_inputs
    proof = qp_wormhole.WormholeProver(config).commit(synthetic_inputs(11, 2)).prove()
    v = qp_wormhole.WormholeVerifier(config)
    v.verify(proof)
    lay = vc.Layout(v.common)
    bad = vc.flip(proof.to_bytes(), lay.tree(3, 1)[0] + 16)
    vd = v.verifier_only + v.common
    assert vc.ora(vd, proof.to_bytes()) == 0
    assert v.verify_batch([proof, bad]) == [0, vc.expect(vc.ora(vd, bad))] == [0, 5]
    with pytest.raises(ValueError, match="proof verification failed: initial merkle path"):
        v.verify(bad)
    v.close()


def test_voting_proofs(ctx):
    """The voting circuit: degree 2^8, one FRI layer, a 16-coefficient final polynomial."""
    import qp_wormhole
    from qp_wormhole.synthetic import synthetic_vote_inputs
    circ = qp_wormhole.Circuit.voting()
    prover = qp_wormhole.Prover(ctx, circ, max_batch=4)
    proofs = prover.prove_witnesses([circ.commit(synthetic_vote_inputs(k, d)) for k, d in ((1, 0), (2, 5), (3, 31))])
    vd, cb = prover.verifier_data(), circ.common_data()
    prover.free()
    v = device_verifier(vd[:len(vd) - len(cb)], cb)
    lay = vc.Layout(cb)
    bad = vc.flip(proofs[1], lay.layer(2, 0)[0] + 5)
    batch = proofs + [bad]
    want = [vc.expect(vc.ora(vd, p)) for p in batch]
    assert want[:3] == [0, 0, 0] and want[3] in (6, 7)
    assert v.verify_batch(batch) == want
    v.close()


def test_aggregation_proof():
    import qp_wormhole
    vo, cb = vc.current_vd()
    l1 = qp_wormhole.aggregate_chunk([golden("dummy_proof.bin"), golden("dummy_proof_zk.bin")], cb, vo)
    cd = l1.circuit_data
    pf, vd = l1.proof.to_bytes(), cd.verifier_data()
    lay = vc.Layout(cd.common)
    bad = vc.flip(pf, lay.openings + 16 * (lay.open_at["wires"] + 50) + 3)
    v = device_verifier(cd.verifier_only, cd.common)
    want = [vc.expect(vc.ora(vd, p)) for p in (pf, bad)]
    assert want == [0, 3]
    assert v.verify_batch([pf, bad]) == want
    v.close()


def test_reference_bench_shape():
    """verifier/benches/verifier.rs on the device: the salted, three-layer circuit."""
    from qp_wormhole import WormholeVerifier
    v = WormholeVerifier.new_from_files(os.path.join(GOLDEN, "verifier.bin"), os.path.join(GOLDEN, "common.bin"))
    v.verify(golden("proof.bin"))
    v.close()
