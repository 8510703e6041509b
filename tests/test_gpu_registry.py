"""VoterRegistry on the device (csrc/registry.hip): the tree, every level and
the compacted paths equal the host fallback's and the oracle loop's
(registry_oracle.py) at the sizes where the kernels can go wrong; proofs from
registry.prove are the bytes of prove_inputs on hand-built inputs.

Sizes: 1, 2, 3; 63, 64, 65 (the wave edge and the one-workgroup fold's
ACC_FOLD_MAX = 64 boundary); 127, 129 (one launch-per-level level above the
fold, odd on both sides); 4097 (several launch-per-level levels, a promoted
node at more than one level, more than one block); 2^16 + 1 (a promoted node
climbing 16 levels)."""
import hashlib

import numpy as np
import pytest

from registry_oracle import oracle_path, oracle_tree, make_keys

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 127, 129, 4097, 2**16 + 1]
BY_HASH = 4097  # from this size on, levels are compared by their SHA-256
PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


_refs = {}


def reference(n):
    """keys, the oracle loop's levels and the host-fallback registry of size n (built once)"""
    if n not in _refs:
        from qp_wormhole import VoterRegistry
        keys = make_keys(n, n)
        _refs[n] = (keys, oracle_tree(keys), VoterRegistry(None, keys))
    return _refs[n]


def sample(n):
    """at most 64 voters: the first, the last two, the 64-aligned ones and their
    neighbours, the rest random"""
    if n <= 64:
        return list(range(n))
    picks = [0, 1, n - 1, n - 2]
    for a in range(64, n, 64):
        picks += [a, a - 1]
    rng = np.random.default_rng(n)
    picks = picks[:48] + [int(x) for x in rng.integers(0, n, 64)]
    return list(dict.fromkeys(picks))[:64]


def sha(levels_array):
    return hashlib.sha256(np.ascontiguousarray(levels_array, dtype=np.uint64).tobytes()).hexdigest()


@pytest.mark.parametrize("n", SIZES)
def test_device_tree_and_paths(ctx, n):
    from qp_wormhole import VoterRegistry
    keys, lv, host = reference(n)
    dev = VoterRegistry(ctx, keys)
    try:
        assert (dev.size, dev.max_depth, dev.num_levels) == (n, host.max_depth, len(lv))
        assert dev.root == host.root == lv[-1][0]
        for l, want in enumerate(lv):
            got = dev.level(l)
            assert got.shape == (len(want), 4), l
            if n >= BY_HASH:
                assert sha(got) == sha(want) == sha(host.level(l)), l
            else:
                assert got.tolist() == want == host.level(l).tolist(), l
        idx = sample(n)
        dsib, dbits, ddepth = dev.paths_raw(idx)
        hsib, hbits, hdepth = host.paths_raw(idx)
        assert np.array_equal(ddepth, hdepth) and np.array_equal(dbits, hbits)
        assert np.array_equal(dsib, hsib)
        sibs, path, depth = dev.paths(idx)
        for b, i in enumerate(idx):
            osib, opath = oracle_path(lv, i)
            assert (sibs[b], path[b], depth[b]) == (osib, opath, len(osib)), i
        if n == 2**16 + 1:  # the promoted node meets its first sibling at the root
            assert depth[idx.index(n - 1)] == 1 and depth[0] == 17
        # refusals on the device path
        with pytest.raises(ValueError, match="outside the registry"):
            dev.paths([n])
    finally:
        dev.free()


def test_abi_refusals(ctx):
    """qp_registry_new / qp_registry_paths refuse what the Python layer checks first"""
    import ctypes
    from qp_wormhole import lib
    from oracle_lib import P
    L = lib()
    h = ctypes.c_void_p()
    good = np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.uint64)
    assert L.qp_registry_new(ctx.h, good, 0, ctypes.byref(h)) == 1 and not h.value
    assert b"no voters" in L.qp_ctx_last_error(ctx.h)
    bad = good.copy()
    bad[2, 1] = P
    assert L.qp_registry_new(ctx.h, bad, 3, ctypes.byref(h)) == 1 and not h.value
    assert b"key 2 felt 1" in L.qp_ctx_last_error(ctx.h)
    assert L.qp_registry_new(ctx.h, good, 2**31 + 1, ctypes.byref(h)) == 1 and not h.value
    assert b"deeper than 31" in L.qp_ctx_last_error(ctx.h)
    assert L.qp_registry_new(ctx.h, good, 3, ctypes.byref(h)) == 0
    try:
        n, d = ctypes.c_uint64(), ctypes.c_uint32()
        assert L.qp_registry_size(h, ctypes.byref(n), ctypes.byref(d)) == 0 and (n.value, d.value) == (3, 2)
        sib, bits, dep = np.zeros((2, 32, 4), np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
        assert L.qp_registry_paths(h, np.array([0, 3], np.uint64), 2, sib, bits, dep) == 1
        assert b"voter index 3" in L.qp_ctx_last_error(ctx.h)
        assert L.qp_registry_paths(h, np.array([2, 1], np.uint64), 2, sib, bits, dep) == 0
        assert dep.tolist() == [1, 2] and bits.tolist() == [1, 1]
    finally:
        L.qp_registry_free(h)


@pytest.fixture(scope="module")
def voting(ctx):
    import qp_wormhole
    circ = qp_wormhole.Circuit.voting()
    prover = qp_wormhole.Prover(ctx, circ, 8)
    yield circ, prover
    prover.free()


def test_prove_voters_end_to_end(ctx, voting):
    from qp_wormhole import VoterRegistry, WormholeVerifier
    from qp_wormhole.prover import _verifier_only
    circ, prover = voting
    keys, lv, host = reference(9)
    voters = [8, 0, 1, 2, 3, 5, 6, 7]
    votes = [bool(i & 1) for i in voters]
    dev = VoterRegistry(ctx, keys)
    try:
        proofs = dev.prove(prover, voters, PROPOSAL, votes)
    finally:
        dev.free()
    hand = [host.inputs(i, PROPOSAL, v) for i, v in zip(voters, votes)]
    assert sorted({x.private_inputs.actual_merkle_depth for x in hand}) == [1, 4]
    assert proofs == prover.prove_inputs(hand)
    assert proofs == host.prove(prover, voters, PROPOSAL, votes)
    ver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=8)
    try:
        assert ver.verify_batch(proofs) == [0] * 8
    finally:
        ver.close()
    for pf, x in zip(proofs, hand):
        pis = [int(v) for v in np.frombuffer(pf[-8 * 13:], np.uint64)]
        assert pis[4:8] == lv[-1][0] and pis[0:4] == PROPOSAL and pis[8] == int(x.public_inputs.vote)
        assert pis[9:13] == x.public_inputs.nullifier


def test_prover_of_another_context_is_refused(voting):
    import qp_wormhole
    from qp_wormhole import QpError, VoterRegistry
    circ, prover = voting
    other = qp_wormhole.Context(0)
    reg = VoterRegistry(other, reference(9)[0])
    try:
        with pytest.raises(QpError, match="QP_ERR_ARG.*another context"):
            reg.prove(prover, [0], PROPOSAL, True)
    finally:
        reg.free()
        other.close()
