"""The commitment-mode VoterRegistry on the device (csrc/registry.hip's update
kernels): after every append and replace the root, every level
(qp_registry_level) and the paths equal the reference's level loop over the
current commitments (registry_open_model.py) and the host fallback taken
through the same steps.

Every sequence runs twice: with the row form forced for every dirty range
(QPGPU_PATHS registry_row=2^31: k_acc_range_row / k_acc_scatter_row
up to the root) and with the one-lane form (registry_row=0: k_acc_level on
a level's suffix, a copy for a lone promoted node, k_acc_scatter, and
k_acc_fold from a level of at most 64 nodes).  Both are compared with the
same model, so they give the same digests.

Beyond the host test's sequences: 1000 -> 1001 -> 1003 -> 1027 (a dirty range
of exactly one node at every level; a range that ends in a promoted node);
(2^16 - 1) -> 2^16 -> (2^16 + 1) (a level kernel hands over to the fold, nlevels
grows, a promoted node climbs 16 levels); replace of 1, 2, 17 and 8193 voters
of 20001 (more than one path batch and scatter block, not a multiple of 16, the
whole-level branch from the level where the batch is no smaller than the
level)."""
import ctypes

import numpy as np
import pytest

from registry_oracle import make_keys
from registry_open_model import (GROWTH, REPLACE_SIZES, check_tree, make_commitments, run_growth, run_replace,
                                 tree_from_leaves)

pytestmark = pytest.mark.gpu

MODES = {"row": "registry_row=2147483648", "one_lane": "registry_row=0"}
PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(params=list(MODES))
def mode(request, monkeypatch):
    monkeypatch.setenv("QPGPU_PATHS", MODES[request.param])
    return request.param


@pytest.mark.parametrize("name", list(GROWTH))
def test_growth(ctx, mode, name):
    run_growth(ctx, name, other_ctx=None)


@pytest.mark.parametrize("n", REPLACE_SIZES)
def test_replace(ctx, mode, n):
    run_replace(ctx, n, other_ctx=None)


_models = {}


def model(key, leaves):
    """the model's levels as arrays, computed once per (case, step) for both modes"""
    if key not in _models:
        _models[key] = [np.array(lv, dtype=np.uint64).reshape(-1, 4) for lv in tree_from_leaves(leaves)]
    return _models[key]


def check_levels(reg, key, leaves, voters):
    from registry_oracle import oracle_path
    lv = model(key, leaves)
    assert (reg.size, reg.num_levels) == (len(leaves), len(lv))
    assert reg.root == lv[-1][0].tolist()
    for l, want in enumerate(lv):
        assert np.array_equal(reg.level(l), want), (key, l)
    lists = [x.tolist() for x in lv]
    sibs, path, depth = reg.paths(voters)
    for b, i in enumerate(voters):
        osib, opath = oracle_path(lists, i)
        assert (sibs[b], path[b], depth[b]) == (osib, opath, len(osib)), (key, i)


@pytest.mark.parametrize("sizes", [[1000, 1001, 1003, 1027], [2**16 - 1, 2**16, 2**16 + 1]], ids=["one-node", "2^16"])
def test_growth_wide(ctx, mode, sizes):
    from qp_wormhole import VoterRegistry
    leaves = make_commitments(sizes[-1], 77)
    reg = VoterRegistry.from_commitments(ctx, leaves[:sizes[0]])
    try:
        check_levels(reg, (sizes[-1], sizes[0]), leaves[:sizes[0]], [0, sizes[0] - 1])
        for n_old, n in zip(sizes, sizes[1:]):
            assert reg.append(leaves[n_old:n]) == n_old
            check_levels(reg, (sizes[-1], n), leaves[:n], [0, n_old - 1, n_old, n - 1])
        if sizes[-1] == 2**16 + 1:  # the promoted node meets its first sibling at the root
            assert reg.paths([2**16])[2] == [1] and reg.num_levels == 18
    finally:
        reg.free()


@pytest.fixture(params=list(MODES) + ["default"])
def mode3(request, monkeypatch):
    if request.param in MODES:
        monkeypatch.setenv("QPGPU_PATHS", MODES[request.param])
    else:
        monkeypatch.delenv("QPGPU_PATHS", raising=False)
    return request.param


def test_replace_batches(ctx, mode3):
    """1, 2, 17 and 8193 voters of 20001, the promoted last voter among them each time"""
    from qp_wormhole import VoterRegistry
    n = 20001
    leaves = make_commitments(n, 5).copy()
    fresh = make_commitments(1 + 2 + 17 + 8193, 6)
    rng = np.random.default_rng(20001)
    reg = VoterRegistry.from_commitments(ctx, leaves, capacity=n)  # the capacity's edge: no spare slot
    try:
        used = 0
        for k in (1, 2, 17, 8193):
            idx = [n - 1] + [int(x) for x in rng.choice(n - 1, k - 1, replace=False)]
            if k == 17:
                idx[1:3] = [4096, 4097]  # both children of one parent
            assert len(set(idx)) == k
            new = fresh[used:used + k]
            used += k
            leaves[idx] = new
            reg.replace(idx, new)
            check_levels(reg, ("replace", k), leaves, idx + [0])  # 8194 paths: two path batches
        assert reg.epoch == 4 and reg.size == n
    finally:
        reg.free()


def test_reserve_and_keyed_equivalence(ctx, mode):
    from qp_wormhole import VoterRegistry
    keys = make_keys(300, 300)
    com = np.array([VoterRegistry.commitment(k) for k in keys], np.uint64)
    keyed = VoterRegistry(ctx, keys)
    reg = VoterRegistry.from_commitments(ctx, com[:129], capacity=129)
    try:
        before = [reg.level(l) for l in range(reg.num_levels)]
        paths = reg.paths_raw(range(129))
        reg.reserve(150)
        assert (reg.capacity, reg.epoch, reg.size) == (150, 1, 129)
        for l, want in enumerate(before):
            assert np.array_equal(reg.level(l), want), l
        for a, b in zip(paths, reg.paths_raw(range(129))):
            assert np.array_equal(a, b)
        assert reg.append(com[129:150], reserve=False) == 129  # fills the capacity exactly
        assert reg.append(com[150:]) == 150  # reserves 300 first
        assert (reg.capacity, reg.epoch, reg.size) == (300, 4, 300)
        assert reg.root == keyed.root and (keyed.capacity, keyed.epoch, keyed.has_keys) == (300, 0, True)
        for l in range(keyed.num_levels):
            assert np.array_equal(reg.level(l), keyed.level(l)), l
    finally:
        reg.free()
        keyed.free()


def test_voting_proof_from_inputs_for(ctx):
    """the proof from a commitment registry's inputs_for is the keyed registry's, byte for byte, and verifies"""
    import qp_wormhole
    from qp_wormhole import VoterRegistry, WormholeVerifier
    from qp_wormhole.prover import _verifier_only
    keys = make_keys(9, 9)
    com = [VoterRegistry.commitment(k) for k in keys]
    circ = qp_wormhole.Circuit.voting()
    prover = qp_wormhole.Prover(ctx, circ, 1)
    keyed = VoterRegistry(ctx, keys)
    reg = VoterRegistry.from_commitments(ctx, com[:5])
    try:
        reg.append(com[5:])
        mine = prover.prove_inputs([reg.inputs_for(keys[8], 8, PROPOSAL, True)])
        assert mine == prover.prove_inputs([keyed.inputs(8, PROPOSAL, True)])
        ver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=1)
        try:
            assert ver.verify_batch(mine) == [0]
        finally:
            ver.close()
        pis = [int(v) for v in np.frombuffer(mine[0][-8 * 13:], np.uint64)]
        assert pis[4:8] == reg.root == keyed.root
        with pytest.raises(ValueError, match="holds no keys"):
            reg.prove(prover, [0], PROPOSAL, True)
        # through the C ABI: QP_ERR_STATE with a message
        from qp_wormhole import lib
        from qp_wormhole.registry import _Ballot
        arr = (_Ballot * 1)()
        arr[0].proposal_id[:] = PROPOSAL
        out = ctypes.create_string_buffer(prover.proof_size)
        ln = (ctypes.c_size_t * 1)()
        rc = lib().qp_prover_prove_voters(prover.h, reg.h, np.array([0], np.uint64), ctypes.cast(arr, ctypes.c_void_p), 1,
                                          out, prover.proof_size, ln)
        assert rc == 4 and b"holds no keys" in lib().qp_ctx_last_error(ctx.h)
    finally:
        reg.free()
        keyed.free()
        prover.free()
        circ.free()


def test_abi_refusals(ctx):
    """the C entry points refuse what the Python layer checks first, and leave the registry as it was"""
    import qp_wormhole
    from qp_wormhole import lib
    from oracle_lib import P
    L = lib()
    err = lambda: L.qp_ctx_last_error(ctx.h)
    h = ctypes.c_void_p()
    good = make_commitments(8, 1)
    dp = lambda a: a.ctypes.data
    assert L.qp_registry_new_commitments(ctx.h, dp(good), 3, 2, ctypes.byref(h)) == 1 and not h.value
    assert b"capacity 2 for 3 voters" in err()
    assert L.qp_registry_new_commitments(ctx.h, dp(good), 3, 2**31 + 1, ctypes.byref(h)) == 1 and not h.value
    assert b"at most 2^31" in err()
    assert L.qp_registry_new_commitments(ctx.h, None, 0, 0, ctypes.byref(h)) == 1 and not h.value
    bad = good.copy()
    bad[2, 1] = P
    assert L.qp_registry_new_commitments(ctx.h, dp(bad), 3, 8, ctypes.byref(h)) == 1 and not h.value
    assert b"commitment 2 (position 2 of the batch) felt 1" in err()
    # an empty registry: no root, paths or level yet
    assert L.qp_registry_new_commitments(ctx.h, None, 0, 4, ctypes.byref(h)) == 0
    root, n, cap, ep = np.zeros(4, np.uint64), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    sib, bits, dep = np.zeros((2, 32, 4), np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.uint32)

    def state():
        assert L.qp_registry_size(h, ctypes.byref(n), None) == 0
        assert L.qp_registry_state(h, ctypes.byref(cap), ctypes.byref(ep)) == 0
        rc = L.qp_registry_root(h, root)
        return n.value, cap.value, ep.value, rc, root.tolist()

    try:
        assert state()[:4] == (0, 4, 0, 4) and b"empty" in err()
        assert L.qp_registry_paths(h, np.array([0], np.uint64), 1, sib, bits, dep) == 4
        assert L.qp_registry_level(h, 0, None, ctypes.byref(n)) == 4
        first = ctypes.c_uint64(99)
        assert L.qp_registry_append(h, dp(good), 0, ctypes.byref(first)) == 0 and first.value == 0
        assert state()[:3] == (0, 4, 0)
        assert L.qp_registry_append(h, dp(good), 3, ctypes.byref(first)) == 0 and first.value == 0
        was = state()
        assert was[:4] == (3, 4, 1, 0)
        # refused, nothing moves
        assert L.qp_registry_append(h, dp(good[3:]), 2, None) == 1
        assert b"exceed the capacity 4" in err() and b"qp_registry_reserve" in err()
        assert L.qp_registry_append(h, dp(bad[2:]), 1, None) == 1 and b"commitment 3 (position 0" in err()
        assert L.qp_registry_replace(h, dp(np.array([0, 3], np.uint64)), dp(good), 2) == 1
        assert b"voter index 3 (position 1) is outside the 3 voters" in err()
        assert L.qp_registry_replace(h, dp(np.array([1, 2, 1], np.uint64)), dp(good), 3) == 1
        assert b"voter index 1 (position 2) appears twice" in err()
        assert L.qp_registry_replace(h, dp(np.array([1, 0, 2], np.uint64)), dp(bad), 3) == 1
        assert b"commitment 2 (position 2 of the batch) felt 1" in err()
        assert L.qp_registry_reserve(h, 2**31 + 1) == 1 and b"at most 2^31" in err()
        assert L.qp_registry_reserve(h, 2) == 1
        assert L.qp_registry_replace(h, dp(np.array([1], np.uint64)), dp(good), 0) == 0
        assert state() == was
        lv = tree_from_leaves(good[:3])
        assert was[4] == lv[-1][0]
        assert L.qp_registry_paths(h, np.array([2, 1], np.uint64), 2, sib, bits, dep) == 0
        assert dep.tolist() == [1, 2] and bits.tolist() == [1, 1]
        # a prover of another context
        other = qp_wormhole.Context(0)
        circ = qp_wormhole.Circuit.voting()
        prover = qp_wormhole.Prover(other, circ, 1)
        try:
            rc = L.qp_prover_prove_voters(prover.h, h, np.array([0], np.uint64), ctypes.cast(root.ctypes.data, ctypes.c_void_p),
                                          1, ctypes.create_string_buffer(8), 8, (ctypes.c_size_t * 1)())
            assert rc == 1 and b"another context" in L.qp_ctx_last_error(other.h)
        finally:
            prover.free()
            circ.free()
            other.close()
    finally:
        L.qp_registry_free(h)
    # a keyed registry refuses the updates
    keys = make_keys(3, 3)
    assert L.qp_registry_new(ctx.h, keys, 3, ctypes.byref(h)) == 0
    try:
        assert L.qp_registry_append(h, dp(good), 1, None) == 4 and b"private keys" in err()
        assert L.qp_registry_replace(h, dp(np.array([0], np.uint64)), dp(good), 1) == 4
        assert L.qp_registry_reserve(h, 8) == 4
        assert L.qp_registry_state(h, ctypes.byref(cap), ctypes.byref(ep)) == 0 and (cap.value, ep.value) == (3, 0)
    finally:
        L.qp_registry_free(h)
