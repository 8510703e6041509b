"""The ballot box's log commitment as a model, from the `Model` of
ballot_model.py and the oracle's hash_no_pad alone: the expected log leaves,
the root at any n, the path of any entry, the answer of `find`, and a
pure-Python receipt checker with the (seq, n) shape rule.  Shared by the
host-path and the device tests; nothing here calls the code under test.

Definitions (include/qpgpu.h): log leaf of entry seq =
hash_no_pad([nullifier[0..4], number, flags]), flags = vote | counted << 1; the
tree over leaves [0, n) in the registry's convention (registry_open_model.
tree_from_leaves); the commitment is (root, n).
"""
import random

import numpy as np

from ballot_model import PROPOSAL, ROOT_A, Model, _homed, ballot, batches, cast_batch, make_stream
from oracle_lib import P, hash_no_pad
from registry_open_model import tree_from_leaves
from registry_oracle import oracle_path

STREAMS = ["distinct", "one_nullifier", "across_batches", "chain_wrap", "felt3_only", "two_keys_shuffled", "screened",
           "grow", "many_blocks"]
SIZES = [1, 2, 3, 5, 65, 131]


def flags_of(entry):
    return int(entry[3]) | int(entry[2]) << 1


def leaf(entry):
    nul, num = entry[0], entry[1]
    return hash_no_pad(list(nul) + [num, flags_of(entry)])


class LogModel:
    """The commitment of a Model's log.  The leaves are hashed once and kept.
    `tree(n)` is the level loop tree_from_leaves over leaves [0, n), from
    scratch (kept per n).  `root(n)` is the same tree read from the top down,
    a plain recursion on the convention's definition: node (l, j) of a tree of
    n leaves is the hash of its two children, or its left child alone where
    the level below ends there.  A node whose leaves all lie below n does not
    depend on n and is kept, so the root at each of a stream's many n costs a
    few hashes; the tests hold root(n) equal to tree(n)'s root where they build
    both."""

    def __init__(self):
        self.leaves, self.levels, self.full = [], {}, {}

    def sync(self, model):
        for e in model.log[len(self.leaves):]:
            self.leaves.append(leaf(e))

    def tree(self, n):
        if n not in self.levels:
            self.levels[n] = tree_from_leaves(self.leaves[:n])
            assert self.levels[n][-1][0] == self.root(n)
        return self.levels[n]

    def _node(self, l, j, n):
        if l == 0:
            return self.leaves[j]
        complete = (j + 1) << l <= n
        if complete and (l, j) in self.full:
            return self.full[l, j]
        below = -(-n // (1 << (l - 1)))  # nodes of level l - 1
        left = self._node(l - 1, 2 * j, n)
        out = hash_no_pad(left + self._node(l - 1, 2 * j + 1, n)) if 2 * j + 1 < below else left
        if complete:
            self.full[l, j] = out
        return out

    def root(self, n):
        assert 1 <= n <= len(self.leaves)
        return self._node((n - 1).bit_length(), 0, n)

    def path(self, seq, n):
        """(siblings, path_bits, depth) of entry seq under the commitment of n entries"""
        sibs, sides = oracle_path(self.tree(n), seq)
        return sibs, sum(int(b) << j for j, b in enumerate(sides)), len(sibs)


def expected_find(model, nullifier):
    """the log index of the counted entry with this nullifier, None if never admitted"""
    num = model.seen.get(tuple(int(x) for x in nullifier))
    if num is None:
        return None
    return next(i for i, e in enumerate(model.log) if e[1] == num)


def shape(seq, n):
    """(depth, path_bits) the tree of n leaves gives entry seq: at level l node
    j = seq >> l has a sibling iff (j ^ 1) < ceil(n / 2^l)"""
    depth = bits = 0
    l, ln = 0, n
    while ln > 1:
        j = seq >> l
        if j ^ 1 < ln:
            bits |= (j & 1) << depth
            depth += 1
        l, ln = l + 1, (ln + 1) // 2
    return depth, bits


def check_receipt(r, root=None, n=None):
    """the receipt check in pure Python over the oracle's hash"""
    root = list(r.root if root is None else root)
    n = r.n if n is None else n
    felts = list(root) + list(r.nullifier) + [r.number] + [x for s in r.siblings for x in s]
    if any(not 0 <= x < P for x in felts):
        return False
    if not 1 <= n <= 1 << 31 or not 0 <= r.seq < n:
        return False
    if (r.depth, r.path_bits) != shape(r.seq, n) or len(r.siblings) != r.depth:
        return False
    cur = hash_no_pad(list(r.nullifier) + [r.number, int(bool(r.vote)) | int(bool(r.counted)) << 1])
    for j, s in enumerate(r.siblings):
        cur = hash_no_pad(list(s) + cur if r.path_bits >> j & 1 else cur + list(s))
    return cur == root


def assert_receipt(r, model, logm, n, check):
    """receipt r of entry r.seq under n entries equals the model's, and both checkers accept it"""
    nul, num, counted, vote = model.log[r.seq]
    sibs, bits, depth = logm.path(r.seq, n)
    assert (tuple(r.nullifier), r.number, r.counted, r.vote) == (nul, num, counted, vote), r.seq
    assert (r.siblings, r.path_bits, r.depth) == (sibs, bits, depth), (r.seq, n)
    assert (r.root, r.n) == (logm.root(n), n)
    assert check_receipt(r) and check(r), (r.seq, n)


def run_commit_stream(box_factory, name, batching, every_batch=True):
    """Casts stream `name` in batches of `batching`; with every_batch commits after
    each batch (and after each reserve) and holds the root to the model's at that
    n, else commits once at the end.  Returns (root, n, model, logm, box): the
    caller frees the box."""
    from qp_wormhole import BallotBox
    cap, roots, items = make_stream(name)
    model, logm = Model(PROPOSAL, roots), LogModel()
    box = box_factory(PROPOSAL, roots, cap)
    try:
        for kind, arg in batches(items, batching):
            if kind == "reserve":
                before = box.commit_log() if every_batch and model.log else None
                box.reserve(arg)
                if before is not None:
                    n = len(model.log)
                    assert box.commit_log() == before == (logm.root(n), n)  # a reserve leaves the root unchanged
                    for r in box.receipts(sorted({0, n - 1, n // 2})):
                        assert_receipt(r, model, logm, n, BallotBox.check_receipt)
                continue
            cast_batch(box, arg)
            for pi, v in arg:
                model.cast_one(pi, v)
            logm.sync(model)
            if every_batch and model.log:
                n = len(model.log)
                assert box.commit_log() == (logm.root(n), n), (name, batching, n)
        n = len(model.log)
        root, got_n = box.commit_log()
        assert (root, got_n) == (logm.root(n), n), (name, batching)
        assert root == logm.tree(n)[-1][0]  # the level loop from scratch
        assert (box.log_root, box.log_size) == (root, n)
    except BaseException:
        box.free()
        raise
    return root, n, model, logm, box


def absent_keys(slots, model):
    """three nullifiers not in the model's log, for a table of `slots` slots
    holding exactly the model's counted nullifiers: one whose home slot is
    empty, one whose home slot starts an occupied chain of other keys, one
    whose chain wraps the table's end (None where the table offers no such
    slot).  The occupancy is recomputed here from the home-slot rule."""
    table = [None] * slots
    for e in model.log:
        if e[2]:
            at = e[0][0] % slots
            while table[at] is not None:
                at = (at + 1) % slots
            table[at] = e[0]
    rng = random.Random("absent")

    def key(home):
        while True:
            k = (_homed(rng, home, slots), rng.randrange(P), rng.randrange(P), rng.randrange(P))
            if k not in model.seen:
                return list(k)
    empty = next((s for s in range(slots) if table[s] is None), None)
    chain = next((s for s in range(slots) if table[s] is not None and table[(s + 1) % slots] is not None
                  and s + 1 < slots), None)
    wrap = slots - 1 if table[slots - 1] is not None and table[0] is not None else None
    return (key(empty) if empty is not None else None, key(chain) if chain is not None else None,
            key(wrap) if wrap is not None else None)


def sized_box(box_factory, n, capacity=None):
    """a box holding n distinct admitted ballots (votes alternate), its model and log model"""
    rng = np.random.default_rng(n)
    nuls = rng.integers(0, P, size=(n, 4), dtype=np.uint64).tolist()
    items = [(ballot(k, i & 1), 0) for i, k in enumerate(nuls)]
    model, logm = Model(PROPOSAL, [ROOT_A]), LogModel()
    box = box_factory(PROPOSAL, model.roots, capacity or n)
    try:
        cast_batch(box, items)
    except BaseException:
        box.free()
        raise
    for pi, v in items:
        model.cast_one(pi, v)
    logm.sync(model)
    return box, model, logm


# ---- the cases both paths run (box_factory(proposal, roots, capacity) makes the box under test)

def check_size(box_factory, n):
    """n admitted entries in a box of exactly that capacity: the root, and the
    receipts of seq 0, n - 1 and n - 2 against the model's paths"""
    from qp_wormhole import BallotBox
    box, model, logm = sized_box(box_factory, n)
    try:
        assert box.commit_log() == (logm.root(n), n) and logm.root(n) == logm.tree(n)[-1][0]
        seqs = sorted({0, n - 1, max(n - 2, 0)})
        rs = box.receipts(seqs)
        assert [r.seq for r in rs] == seqs
        for r in rs:
            assert_receipt(r, model, logm, n, BallotBox.check_receipt)
        return [tuple(r) for r in rs]
    finally:
        box.free()


def check_find(box_factory):
    """find on the streams with doubles, a wrapped chain and keys equal in the
    home-slot felt; absent keys of the three kinds; batches of 1 and 300; a
    felt = p refused"""
    import pytest
    from qp_wormhole import QpError
    answers = {}
    for name in ("across_batches", "chain_wrap", "felt3_only", "two_keys_shuffled", "grow"):
        cap, roots, items = make_stream(name)
        model = Model(PROPOSAL, roots)
        box = box_factory(PROPOSAL, roots, cap)
        try:
            for kind, arg in batches(items, 7):
                if kind == "reserve":
                    box.reserve(arg)
                    cap = arg
                    continue
                cast_batch(box, arg)
                for pi, v in arg:
                    model.cast_one(pi, v)
            # every entry's nullifier, doubles included: the counted entry's index, never the double's own
            queries = [list(e[0]) for e in model.log]
            want = [expected_find(model, q) for q in queries]
            assert all(model.log[w][2] for w in want)
            assert any(w != i for i, w in enumerate(want)) or name == "felt3_only"
            got = box.find(queries)
            assert got == want, name
            assert box.find([queries[-1]]) == [want[-1]]  # a batch of one
            slots = 2
            while slots < 2 * cap:
                slots *= 2
            absent = absent_keys(slots, model)
            if name == "chain_wrap":
                assert None not in absent  # this stream's table has all three kinds
            absent = [a for a in absent if a is not None]
            assert box.find(absent) == [None] * len(absent), name
            # 300 queries: more than one block with a ragged tail; present and absent mixed
            mixed = [(queries[i % len(queries)] if i % 3 else absent[i % len(absent)]) for i in range(300)]
            got300 = box.find(mixed)
            assert got300 == [expected_find(model, q) for q in mixed], name
            assert box.find([]) == []
            bad = [queries[0], queries[1][:2] + [P] + queries[1][3:]]
            with pytest.raises(QpError, match="QP_ERR_ARG.*position 1"):
                box.find(bad)
            answers[name] = (got, got300)
        finally:
            box.free()
    return answers


def tampered(r, other, last):
    """(what, receipt) pairs that must not check; `other`: another receipt of the
    same commitment; `last`: the receipt of its last entry.  n enters the check
    through the tree's shape alone (the root binds the content), so a wrong n
    shows where it changes the shape of the receipt's seq: at the last entry,
    whose node n + 1 leaves would hash and n leaves promote, and below seq."""
    sib = [list(d) for d in r.siblings]
    sib[-1][2] ^= 1
    out = [("vote", r._replace(vote=not r.vote)), ("counted", r._replace(counted=not r.counted)),
           ("number", r._replace(number=r.number + 1)), ("sibling felt", r._replace(siblings=sib)),
           ("depth + 1", r._replace(depth=r.depth + 1, siblings=r.siblings + [[0, 0, 0, 0]])),
           ("depth - 1", r._replace(depth=r.depth - 1, siblings=r.siblings[:-1])),
           ("path bit", r._replace(path_bits=r.path_bits ^ 1)),
           ("top path bit", r._replace(path_bits=r.path_bits ^ (1 << (r.depth - 1)))),
           ("wrong n", last._replace(n=last.n + 1)), ("n at seq", last._replace(n=last.n - 1)),
           ("n = 0", r._replace(n=0)), ("n twice", r._replace(n=2 * r.n)),
           ("another entry's seq", r._replace(seq=other.seq)),
           ("non-canonical sibling", r._replace(siblings=[[P, 0, 0, 0]] + r.siblings[1:]))]
    return out


def check_receipt_rules(box_factory):
    """a double's own receipt, every tampering, a receipt offered against a later
    commitment, and the refusals"""
    import pytest
    from qp_wormhole import BallotBox, QpError
    cap, roots, items = make_stream("across_batches")
    model, logm = Model(PROPOSAL, roots), LogModel()
    box = box_factory(PROPOSAL, roots, cap)
    try:
        with pytest.raises(QpError, match="QP_ERR_STATE.*empty log"):
            box.commit_log()
        with pytest.raises(QpError, match="QP_ERR_STATE.*empty log"):
            box.receipts([0])
        half = items[:37]  # 32 counted ballots and five doubles
        cast_batch(box, half)
        for pi, v in half:
            model.cast_one(pi, v)
        logm.sync(model)
        n_a = len(model.log)
        pair = box.commit_log()
        assert pair == (logm.root(n_a), n_a) and box.commit_log() == pair  # nothing new: the same pair
        double = box.receipts([34])[0]  # a double vote's own entry
        assert not double.counted and double.seq == 34
        assert_receipt(double, model, logm, n_a, BallotBox.check_receipt)
        assert box.receipt_for(double.nullifier).seq == 2 and box.receipt_for([1, 2, 3, 4]) is None
        r, other, last = box.receipts([5, 20, n_a - 1])
        for x in (r, other, last):
            assert_receipt(x, model, logm, n_a, BallotBox.check_receipt)
        for what, bad in tampered(r, other, last):
            assert not BallotBox.check_receipt(bad), what
            assert not check_receipt(bad), what
        with pytest.raises(QpError, match="QP_ERR_ARG.*position 1"):
            box.receipts([0, n_a])
        assert box.commit_log() == pair
        # a later commitment: the old receipt holds under its own pair only
        cast_batch(box, items[37:])
        for pi, v in items[37:]:
            model.cast_one(pi, v)
        logm.sync(model)
        n_b = len(model.log)
        root_b, got_n = box.commit_log()
        assert (root_b, got_n) == (logm.root(n_b), n_b) and root_b != pair[0]
        assert BallotBox.check_receipt(r) and BallotBox.check_receipt(r, pair[0], n_a)
        for root, n in ((root_b, n_b), (root_b, n_a)):
            assert not BallotBox.check_receipt(r, root, n) and not check_receipt(r, root, n)
        again = box.receipts([5])[0]
        assert_receipt(again, model, logm, n_b, BallotBox.check_receipt)
        return [tuple(x) for x in (double, r, other, again)]
    finally:
        box.free()
