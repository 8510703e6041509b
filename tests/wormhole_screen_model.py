"""The input screen's rules in a few lines of Python over the oracle's
hash_no_pad (oracle_lib), and the table of cases every path is held to: the
library's host path (test_input_screen.py), the device path and, case by case,
the circuit itself through the unchanged prove_inputs (test_gpu_input_screen.py).

A case is (name, CircuitInputs, (status, witness)): the expectation is written
down by hand per case, and test_input_screen.py checks that the model gives it.
The tries are built here (build): node i holds the digest of node i + 1 as eight
little-endian u32 limbs at a chosen felt, the last node holds the leaf hash."""
import copy
import random
import struct

from oracle_lib import hash_no_pad as _oracle_hash

from qp_wormhole import CircuitInputs, PrivateCircuitInputs, ProcessedStorageProof, PublicCircuitInputs

P = 0xFFFFFFFF00000001
M32 = 0xFFFFFFFF
OK, FIELD_RANGE, PROOF_TOO_LONG, NODE_TOO_LARGE, NULLIFIER, UNSPENDABLE, STORAGE_NODE, STORAGE_LEAF = range(8)
MAX_NODES, NODE_FELTS, SCAN_STARTS = 20, 188, 180

_memo = {}


def H(v):
    """hash_n_to_hash_no_pad; every digest is computed once and shared by the tests"""
    k = tuple(v)
    if k not in _memo:
        _memo[k] = _oracle_hash(list(k))
    return _memo[k]


def felts(b):
    """4-byte little-endian limbs, a short last limb zero-extended"""
    return [int.from_bytes(b[i:i + 4], "little") for i in range(0, len(b), 4)]


def digest(b):
    return [int.from_bytes(b[8 * i:8 * i + 8], "little") for i in range(4)]


def digest_bytes(d):
    return b"".join(struct.pack("<Q", x) for x in d)


def count_felts(c):
    return [c >> 32, c & M32]


def amount_felts(a):
    return [(a >> (96 - 32 * i)) & M32 for i in range(4)]


def node_felts(node):
    f = felts(node)
    return f + [0] * (NODE_FELTS - len(f))


def leaf_hash(x):
    return H(count_felts(x.private.transfer_count) + digest(x.private.funding_account) +
             digest(x.private.unspendable_account) + amount_felts(x.public.funding_amount))


def model(x):
    """(status, witness) of CircuitInputs x: the first check that fails"""
    pub, prv = x.public, x.private
    for k, d in enumerate((pub.nullifier, prv.unspendable_account, pub.root_hash, prv.funding_account,
                           pub.exit_account)):
        if any(v >= P for v in digest(d)):
            return FIELD_RANGE, k
    nodes, indices = prv.storage_proof.proof, prv.storage_proof.indices
    if len(nodes) > MAX_NODES:
        return PROOF_TOO_LONG, len(nodes)
    for i, nd in enumerate(nodes):
        if len(nd) > 4 * NODE_FELTS:
            return NODE_TOO_LARGE, i
    count = count_felts(prv.transfer_count)
    if H(H(felts(b"~nullif~") + felts(prv.secret) + count)) != digest(pub.nullifier):
        return NULLIFIER, 0
    if H(H(felts(b"wormhole") + felts(prv.secret))) != digest(prv.unspendable_account):
        return UNSPENDABLE, 0
    due = digest(pub.root_hash)
    for i, nd in enumerate(nodes):
        f = node_felts(nd)
        if H(f) != due:
            return STORAGE_NODE, i
        s = indices[i] // 8
        due = [(f[s + 2 * y] + (f[s + 2 * y + 1] << 32)) % P for y in range(4)] if s < SCAN_STARTS else [0] * 4
    if len(nodes) < MAX_NODES and leaf_hash(x)[1:] != due[1:]:
        return STORAGE_LEAF, len(nodes)
    return OK, 0


# ---------------------------------------------------------------- the case builder

def _felt_bytes(r):
    return digest_bytes([r.randrange(P) for _ in range(4)])


def build(depth, seed, lens=None, starts=None, hex_off=None, embed=None):
    """A consistent input with a trie of `depth` nodes: lens[i] bytes in node i (default 240),
    the child digest at felt starts[i] (default 3) of node i, indices[i] = 8 * starts[i] +
    hex_off[i] (default 0).  embed(leaf hash) -> the four felts the last node (the root at
    depth 0) holds in the leaf hash's place.  A digest that does not fit below lens[i] is not
    written (the node then simply does not hold it)."""
    r = random.Random(0x5C4EE7 + seed)
    lens = lens or [240] * depth
    starts = starts or [3] * depth
    hex_off = hex_off or [0] * depth
    secret = r.randbytes(32)
    count = r.getrandbits(64)
    amount = r.getrandbits(128)
    funding, exit_account = _felt_bytes(r), _felt_bytes(r)
    unspendable = digest_bytes(H(H(felts(b"wormhole") + felts(secret))))
    nullifier = digest_bytes(H(H(felts(b"~nullif~") + felts(secret) + count_felts(count))))
    leaf = H(count_felts(count) + digest(funding) + digest(unspendable) + amount_felts(amount))
    child = list(embed(leaf)) if embed else leaf
    nodes, indices = [None] * depth, [0] * depth
    for i in reversed(range(depth)):
        body = bytearray(r.randbytes(lens[i]))
        if 4 * starts[i] + 32 <= lens[i]:
            body[4 * starts[i]:4 * starts[i] + 32] = b"".join(struct.pack("<II", h & M32, h >> 32) for h in child)
        nodes[i], indices[i] = bytes(body), 8 * starts[i] + hex_off[i]
        child = H(node_felts(nodes[i]))
    return CircuitInputs(PublicCircuitInputs(amount, nullifier, digest_bytes(child), exit_account),
                         PrivateCircuitInputs(secret, ProcessedStorageProof(nodes, indices), count, funding, unspendable))


def _with(x, **kw):
    """a deep copy of x with public / private fields replaced; node=(i, bytes), index=(i, int)"""
    y = copy.deepcopy(x)
    for k, v in kw.items():
        if k == "node":
            y.private.storage_proof.proof[v[0]] = v[1]
        elif k == "index":
            y.private.storage_proof.indices[v[0]] = v[1]
        elif hasattr(y.public, k):
            setattr(y.public, k, v)
        else:
            setattr(y.private, k, v)
    return y


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]


def _flip_node(x, i, at):
    return _with(x, node=(i, _flip(x.private.storage_proof.proof[i], at)))


def _out_of_range(b, chunk, value=P):
    return b[:8 * chunk] + struct.pack("<Q", value) + b[8 * chunk + 8:]


def _cases():
    c = []

    def add(name, x, status, witness=0):
        c.append((name, x, (status, witness)))

    # depths 0, 1, 2, 19, 20; node lengths 32 (a bare digest), 61 (a short last limb), 720, 752; the child
    # digest at felt 0, at felt 179 (the last start the circuit scans), a hex index that is no multiple of 8
    d0, d1 = build(0, 1), build(1, 2, lens=[32], starts=[0])
    d2 = build(2, 3, lens=[61, 752], starts=[7, 179], hex_off=[5, 7])
    d5 = build(5, 4, lens=[720, 32, 240, 61, 752], starts=[172, 0, 20, 2, 179], hex_off=[0, 3, 0, 1, 0])
    d19 = build(19, 5, lens=[64 + 36 * i for i in range(19)], starts=[i % 9 for i in range(19)])
    d20 = build(20, 6, lens=[752 - 32 * i for i in range(20)], starts=[(7 * i) % 28 for i in range(20)])
    for name, x in (("depth0", d0), ("depth1_len32_felt0", d1), ("depth2_len61_len752_felt179_hexoff", d2),
                    ("depth5_mixed_lengths", d5), ("depth19", d19), ("depth20", d20)):
        add(name, x, OK)
    # a node is hashed zero-padded: zero bytes appended to it change nothing
    add("zero_bytes_appended", _with(d5, node=(2, d5.private.storage_proof.proof[2] + bytes(9))), OK)

    # a felt start >= 180 finds the zero digest: bad at the next position, though the node holds the digest there
    far_mid = build(3, 7, lens=[240, 752, 240], starts=[3, 180, 3])
    far_last = build(3, 8, lens=[240, 240, 752], starts=[3, 3, 180])
    add("start180_middle_node", far_mid, STORAGE_NODE, 2)
    add("start180_last_node", far_last, STORAGE_LEAF, 3)
    add("start_huge_index", _with(d5, index=(1, (1 << 64) - 1)), STORAGE_NODE, 2)
    # the same nodes with the start the digest really is at, one felt lower, are fine
    add("start179_last_node", build(3, 8, lens=[240, 240, 752], starts=[3, 3, 179]), OK)

    # one byte flipped: node 0, a middle node, the last node, inside the embedded digest
    add("flip_node0", _flip_node(d5, 0, 700), STORAGE_NODE, 0)
    add("flip_middle_node", _flip_node(d5, 2, 5), STORAGE_NODE, 2)
    add("flip_last_node", _flip_node(d5, 4, 40), STORAGE_NODE, 4)
    add("flip_embedded_digest", _flip_node(d5, 2, 4 * 20 + 9), STORAGE_NODE, 2)
    add("flip_depth20_last_node", _flip_node(d20, 19, 0), STORAGE_NODE, 19)
    add("flip_short_last_limb", _flip_node(d2, 0, 60), STORAGE_NODE, 0)
    add("wrong_index", _with(d5, index=(2, 8 * 21)), STORAGE_NODE, 3)
    add("wrong_root", _with(d5, root_hash=_flip(d5.public.root_hash, 3)), STORAGE_NODE, 0)

    # felt 0 of the leaf hash is not compared; felt 1 is
    add("leaf_felt0_differs", build(3, 9, embed=lambda h: [h[0] ^ 1] + h[1:]), OK)
    add("leaf_felt1_differs", build(3, 9, embed=lambda h: [h[0], h[1] ^ 1] + h[2:]), STORAGE_LEAF, 3)
    add("leaf_felt3_differs", build(19, 10, embed=lambda h: h[:3] + [h[3] ^ (1 << 40)]), STORAGE_LEAF, 19)
    add("depth0_root_felt0_differs", _with(d0, root_hash=_flip(d0.public.root_hash, 0)), OK)
    add("depth0_root_felt1_differs", _with(d0, root_hash=_flip(d0.public.root_hash, 8)), STORAGE_LEAF, 0)
    # at depth 20 no leaf check exists at all
    add("depth20_wrong_leaf", build(20, 11, embed=lambda h: [x ^ 1 for x in h]), OK)
    add("depth20_wrong_amount", _with(d20, funding_amount=d20.public.funding_amount ^ 1), OK)

    # wrong values
    add("wrong_nullifier", _with(d5, nullifier=_flip(d5.public.nullifier, 17)), NULLIFIER)
    add("wrong_secret", _with(d5, secret=_flip(d5.private.secret, 31)), NULLIFIER)
    add("wrong_unspendable", _with(d5, unspendable_account=_flip(d5.private.unspendable_account, 2)), UNSPENDABLE)
    add("wrong_amount", _with(d5, funding_amount=d5.public.funding_amount ^ (1 << 127)), STORAGE_LEAF, 5)
    add("wrong_amount_depth0", _with(d0, funding_amount=d0.public.funding_amount ^ 1), STORAGE_LEAF, 0)
    add("wrong_funding_account", _with(d5, funding_account=_flip(d5.private.funding_account, 9)), STORAGE_LEAF, 5)
    # a wrong transfer count is the nullifier's fault first, though the leaf is wrong too
    add("wrong_transfer_count", _with(d5, transfer_count=d5.private.transfer_count ^ (1 << 32)), NULLIFIER)
    # the exit account is unconstrained
    add("wrong_exit_account", _with(d5, exit_account=_flip(d5.public.exit_account, 1)), OK)

    # statuses 1-3, each with its witness
    for k, fld in enumerate(("nullifier", "unspendable_account", "root_hash", "funding_account", "exit_account")):
        src = d5.public if hasattr(d5.public, fld) else d5.private
        add(f"range_{fld}", _with(d5, **{fld: _out_of_range(getattr(src, fld), k % 4)}), FIELD_RANGE, k)
    add("range_top_value", _with(d5, root_hash=_out_of_range(d5.public.root_hash, 3, (1 << 64) - 1)), FIELD_RANGE, 2)
    add("range_p_minus_1_is_fine", _with(d0, exit_account=_out_of_range(d0.public.exit_account, 0, P - 1)), OK)
    long21 = copy.deepcopy(d20)
    long21.private.storage_proof.proof.append(bytes(40))
    long21.private.storage_proof.indices.append(0)
    add("proof_21_nodes", long21, PROOF_TOO_LONG, 21)
    add("node_753_bytes", _with(d5, node=(2, d5.private.storage_proof.proof[2] + bytes(753 - 240))), NODE_TOO_LARGE, 2)
    add("node_752_bytes_zero_tail", _with(d5, node=(2, d5.private.storage_proof.proof[2] + bytes(752 - 240))), OK)

    # two faults in one input: the lower status, the lower witness
    both_range = _with(d5, exit_account=_out_of_range(d5.public.exit_account, 1),
                       unspendable_account=_out_of_range(d5.private.unspendable_account, 2))
    add("two_range_faults", both_range, FIELD_RANGE, 1)
    add("range_and_too_long", _with(long21, funding_account=_out_of_range(d20.private.funding_account, 0)),
        FIELD_RANGE, 3)
    add("too_long_and_too_large", _with(long21, node=(4, bytes(800))), PROOF_TOO_LONG, 21)
    add("too_large_and_wrong_nullifier", _with(d5, node=(3, bytes(1000)), nullifier=_flip(d5.public.nullifier, 0)),
        NODE_TOO_LARGE, 3)
    add("nullifier_and_unspendable", _with(d5, nullifier=_flip(d5.public.nullifier, 0),
                                           unspendable_account=_flip(d5.private.unspendable_account, 0)), NULLIFIER)
    add("unspendable_and_node", _flip_node(_with(d5, unspendable_account=_flip(d5.private.unspendable_account, 0)), 1, 3),
        UNSPENDABLE)
    add("two_flipped_nodes", _flip_node(_flip_node(d5, 3, 8), 1, 30), STORAGE_NODE, 1)
    add("node_and_amount", _flip_node(_with(d5, funding_amount=d5.public.funding_amount ^ 2), 4, 100), STORAGE_NODE, 4)
    return c


CASES = _cases()
CASE_IDS = [name for name, _, _ in CASES]


def mixed_batch(n):
    """n inputs of mixed depth and verdict drawn from the cases that have their storage-proof arrays in
    order (status 1-3 included), with a bad one in the first and in the last position"""
    bad = [x for _, x, want in CASES if want[0] >= NULLIFIER]
    pool = [x for _, x, _ in CASES]
    xs = [pool[(5 * i + 1) % len(pool)] for i in range(n)]
    xs[0], xs[-1] = bad[0], bad[-1 if n > 1 else 0]
    return xs
