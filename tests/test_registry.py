"""VoterRegistry on the host fallback (no device): the reference's tree
convention (voting/src/lib.rs:285-316: leaf = H(key), node = H(left || right),
the last node of an odd level promoted unchanged), the compacted paths the
voting circuit walks (:123-180), the refusals, and the circuit accepting every
path.  The checker is the oracle's hash_no_pad through registry_oracle.py."""
import dataclasses

import pytest

import qp_wormhole
from qp_wormhole import QpError, VoterRegistry
from qp_wormhole.synthetic import bytes_to_digest, vote_test_inputs
from oracle_lib import P, hash_no_pad
from registry_oracle import oracle_path, oracle_tree, root_from_path, make_keys

PROPOSAL = bytes_to_digest(bytes([42] * 32))


@pytest.fixture(scope="module")
def circuit():
    c = qp_wormhole.Circuit.voting()
    yield c
    c.free()


def test_reference_tree():
    """create_test_inputs (voting/src/lib.rs:285-343): the four-key tree, voter 0."""
    keys = [bytes_to_digest(bytes([k] * 32)) for k in (1, 2, 3, 4)]
    reg = VoterRegistry(None, keys)
    ref = vote_test_inputs()
    got = reg.inputs(0, PROPOSAL, True)
    lv = oracle_tree(keys)
    assert reg.size == 4 and reg.max_depth == 2
    assert reg.root == lv[2][0] == ref.public_inputs.merkle_root
    for f in dataclasses.fields(ref.public_inputs):
        assert getattr(got.public_inputs, f.name) == getattr(ref.public_inputs, f.name), f.name
    for f in dataclasses.fields(ref.private_inputs):
        assert getattr(got.private_inputs, f.name) == getattr(ref.private_inputs, f.name), f.name
    assert got.private_inputs.merkle_siblings == [lv[0][1], lv[1][1]]
    assert got.private_inputs.path_indices == [False, False]
    assert got.private_inputs.actual_merkle_depth == 2


def test_single_voter():
    key = [[5, 6, 7, P - 1]]
    reg = VoterRegistry(None, key)
    sibs, path, depth = reg.paths([0])
    assert (reg.size, reg.max_depth, depth, sibs, path) == (1, 0, [0], [[]], [[]])
    assert reg.root == hash_no_pad(key[0])


@pytest.mark.parametrize("n", [2, 3, 5, 6, 7, 9])
def test_odd_sizes(n):
    keys = make_keys(n, n)
    reg = VoterRegistry(None, keys)
    lv = oracle_tree(keys)
    assert reg.root == lv[-1][0]
    assert reg.num_levels == len(lv) and reg.max_depth == len(lv) - 1
    for l, want in enumerate(lv):
        assert reg.level(l).tolist() == want, l
    sibs, path, depth = reg.paths(range(n))
    raw_sib, raw_bits, raw_depth = reg.paths_raw(range(n))
    for i in range(n):
        osib, opath = oracle_path(lv, i)
        assert depth[i] == len(osib) == int(raw_depth[i]), i
        assert sibs[i] == osib and path[i] == opath, i
        assert root_from_path(keys[i], sibs[i], path[i]) == reg.root, i
        assert not raw_sib[i, depth[i]:].any() and int(raw_bits[i]) >> depth[i] == 0, i
    if n == 3:
        assert depth == [2, 2, 1]
    if n == 5:
        assert depth == [3, 3, 3, 3, 1]


def test_refusals():
    with pytest.raises(ValueError, match="at least one voter"):
        VoterRegistry(None, [])
    with pytest.raises(ValueError, match="key 1 felt 2 is not a canonical field element"):
        VoterRegistry(None, [[1, 2, 3, 4], [1, 2, P, 4]])
    with pytest.raises(ValueError, match="key 0 felt 0"):
        VoterRegistry(None, [[2**64 - 1, 0, 0, 0]])
    reg = VoterRegistry(None, make_keys(5))
    for call in (lambda: reg.paths([5]), lambda: reg.paths([0, -1]), lambda: reg.inputs(5, PROPOSAL, True),
                 lambda: reg.paths_raw([2**40])):
        with pytest.raises(ValueError, match="outside the registry's 5 voters"):
            call()
    with pytest.raises(ValueError, match="proposal_id"):
        reg.inputs(0, [1, 2, 3, P], True)


@pytest.mark.parametrize("n", [5, 6])
def test_circuit_accepts_every_path(circuit, n):
    """commit() runs the circuit's own Merkle walk over the compacted path."""
    reg = VoterRegistry(None, make_keys(n, 40 + n))
    for i in range(n):
        inp = reg.inputs(i, PROPOSAL, bool(i & 1))
        w = circuit.commit(inp)
        pis = [int(x) for x in w.public_inputs()]
        assert pis[4:8] == reg.root, i
        w.free()
    # one sibling flipped: the walk ends at another root
    inp = reg.inputs(0, PROPOSAL, True)
    inp.private_inputs.merkle_siblings[1][2] ^= 1
    with pytest.raises(QpError, match="set twice"):
        circuit.commit(inp)
