"""The commitment-mode VoterRegistry on the host fallback (no device):
from_commitments, append, replace and reserve against the reference's level
loop over the current commitments (registry_open_model.py), the refusals (each
leaving root, size and epoch as they were), and inputs_for.

The host fallback applies the same dirty-range rule as the device (level l of
an append changes in [n_old >> l, ceil(n / 2^l))), so the sequences are the
smallest that reach each of its branches: see GROWTH in the model file."""
import numpy as np
import pytest

import qp_wormhole
from qp_wormhole import VoterRegistry
from oracle_lib import P, hash_no_pad
from registry_oracle import make_keys, root_from_path
from registry_open_model import GROWTH, REPLACE_SIZES, check_tree, make_commitments, run_growth, run_replace

PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4


@pytest.mark.parametrize("name", list(GROWTH))
def test_growth(name):
    run_growth(None, name)


@pytest.mark.parametrize("n", REPLACE_SIZES)
def test_replace(n):
    run_replace(None, n)


@pytest.mark.parametrize("n", [1, 5, 64, 131])
def test_keyed_equivalence(n):
    keys = make_keys(n, n)
    keyed = VoterRegistry(None, keys)
    reg = VoterRegistry.from_commitments(None, [VoterRegistry.commitment(k) for k in keys])
    assert VoterRegistry.commitment(keys[0]) == hash_no_pad([int(x) for x in keys[0]])
    assert reg.root == keyed.root and reg.num_levels == keyed.num_levels
    for l in range(keyed.num_levels):
        assert reg.level(l).tolist() == keyed.level(l).tolist(), l
    assert keyed.has_keys and (keyed.capacity, keyed.epoch) == (n, 0)
    assert not reg.has_keys


def snapshot(reg):
    return reg.root, reg.size, reg.epoch, reg.capacity, [reg.level(l).tolist() for l in range(reg.num_levels)]


def test_refusals_leave_the_registry_as_it_was():
    leaves = make_commitments(9, 3)
    reg = VoterRegistry.from_commitments(None, leaves[:5], capacity=6)
    before = snapshot(reg)
    bad = leaves[5:8].copy()
    bad[1, 2] = P
    with pytest.raises(ValueError, match=r"commitment 6 \(position 1 of the batch\) felt 2 is not a canonical"):
        reg.append(bad)
    with pytest.raises(ValueError, match="outside the registry's 5 voters"):
        reg.replace([0, 5], leaves[5:7])
    with pytest.raises(ValueError, match=r"voter index 3 \(position 2\) appears twice"):
        reg.replace([3, 1, 3], leaves[5:8])
    with pytest.raises(ValueError, match=r"commitment 4 \(position 1 of the batch\) felt 2"):
        reg.replace([0, 4, 2], bad)
    with pytest.raises(ValueError, match="5 \\+ 2 voters exceed the capacity 6; call reserve"):
        reg.append(leaves[5:7], reserve=False)
    with pytest.raises(ValueError, match="at most 2\\^31"):
        reg.reserve(2**31 + 1)
    with pytest.raises(ValueError, match="must hold them"):
        reg.reserve(4)
    with pytest.raises(ValueError, match="holds no keys"):
        reg.inputs(0, PROPOSAL, True)
    with pytest.raises(ValueError, match="holds no keys"):
        reg.prove(None, [0], PROPOSAL, True)
    assert reg.append([]) == 5 and snapshot(reg) == before  # k == 0: nothing changes
    reg.replace([], [])
    assert snapshot(reg) == before
    # the Python append reserves instead of refusing
    assert reg.append(leaves[5:7]) == 5
    assert (reg.size, reg.capacity, reg.epoch) == (7, 12, 2)  # one reserve, one append
    check_tree(reg, leaves[:7], [0, 4, 5, 6])
    with pytest.raises(ValueError, match="at most 2\\^31"):
        VoterRegistry.from_commitments(None, leaves, capacity=2**31 + 1)
    with pytest.raises(ValueError, match="must hold them"):
        VoterRegistry.from_commitments(None, leaves, capacity=8)
    with pytest.raises(ValueError, match="commitment 2 .* felt 0"):
        VoterRegistry.from_commitments(None, [[1, 2, 3, 4], [5, 6, 7, 8], [P, 0, 0, 0]])


def test_empty_registry():
    reg = VoterRegistry.from_commitments(None, [])
    assert (reg.size, reg.root, reg.capacity, reg.epoch, reg.num_levels) == (0, None, 1024, 0, 0)
    with pytest.raises(ValueError, match="registry is empty"):
        reg.paths([0])
    with pytest.raises(ValueError, match="registry is empty"):
        reg.paths([])
    with pytest.raises(ValueError, match="registry is empty"):
        reg.level(0)
    assert (reg.size, reg.root, reg.epoch) == (0, None, 0)


def test_keyed_registry_refuses_updates():
    keys = make_keys(5, 1)
    reg = VoterRegistry(None, keys)
    root = list(reg.root)
    for call in (lambda: reg.append(make_commitments(2)), lambda: reg.replace([0], make_commitments(1)),
                 lambda: reg.reserve(16)):
        with pytest.raises(ValueError, match="built from private keys"):
            call()
    assert (reg.root, reg.size, reg.epoch, reg.capacity) == (root, 5, 0, 5)


def test_reserve_keeps_levels_and_paths():
    leaves = make_commitments(40, 5)
    reg = VoterRegistry.from_commitments(None, leaves[:21], capacity=21)
    lv = check_tree(reg, leaves[:21], range(21))
    paths = reg.paths_raw(range(21))
    reg.reserve(64)
    assert (reg.capacity, reg.epoch, reg.size) == (64, 1, 21)
    assert check_tree(reg, leaves[:21], range(21)) == lv
    for a, b in zip(paths, reg.paths_raw(range(21))):
        assert np.array_equal(a, b)
    reg.reserve(64)  # the same capacity: nothing to do
    assert reg.epoch == 1
    assert reg.append(leaves[21:40], reserve=False) == 21
    check_tree(reg, leaves, [0, 20, 21, 39])
    reg.reserve(40)  # down to the size
    assert (reg.capacity, reg.epoch) == (40, 3)
    check_tree(reg, leaves, [0, 39])


def test_inputs_for():
    n = 9
    keys = make_keys(n, 9)
    reg = VoterRegistry.from_commitments(None, [VoterRegistry.commitment(k) for k in keys[:4]])
    reg.append([VoterRegistry.commitment(k) for k in keys[4:]])
    keyed = VoterRegistry(None, keys)
    for i in (0, 4, n - 1):  # the first, a middle and the promoted last voter
        x = reg.inputs_for(keys[i], i, PROPOSAL, i & 1)
        pv = x.private_inputs
        assert root_from_path(pv.private_key, pv.merkle_siblings, pv.path_indices) == reg.root
        assert x.public_inputs.merkle_root == reg.root == keyed.root
        want = keyed.inputs(i, PROPOSAL, i & 1)
        assert (x.public_inputs, x.private_inputs) == (want.public_inputs, want.private_inputs)
    assert reg.inputs_for(keys[n - 1], n - 1, PROPOSAL, True).private_inputs.actual_merkle_depth == 1
    with pytest.raises(ValueError, match="not the one voter 3 registered"):
        reg.inputs_for(keys[2], 3, PROPOSAL, True)
    with pytest.raises(ValueError, match="outside the registry's 9 voters"):
        reg.inputs_for(keys[0], 9, PROPOSAL, True)
    # a keyed registry serves a voter's own key the same way
    assert keyed.inputs_for(keys[1], 1, PROPOSAL, False).private_inputs == keyed.inputs(1, PROPOSAL, False).private_inputs


def test_circuit_accepts_a_path_after_updates():
    """commit() runs the circuit's own Merkle walk over a path taken after an append and a replace"""
    keys = make_keys(7, 21)
    reg = VoterRegistry.from_commitments(None, [VoterRegistry.commitment(k) for k in keys[:3]])
    reg.append([VoterRegistry.commitment(k) for k in keys[3:6]])
    reg.replace([1], [VoterRegistry.commitment(keys[6])])  # voter 1 struck off, the seat given to key 6
    circ = qp_wormhole.Circuit.voting()
    try:
        for key, i in ((keys[6], 1), (keys[5], 5)):
            w = circ.commit(reg.inputs_for(key, i, PROPOSAL, True))
            assert [int(x) for x in w.public_inputs()][4:8] == reg.root
            w.free()
    finally:
        circ.free()
    with pytest.raises(ValueError, match="not the one voter 1 registered"):
        reg.inputs_for(keys[1], 1, PROPOSAL, True)
