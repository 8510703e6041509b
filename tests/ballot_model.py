"""The ballot box's semantics as a model (a dict from nullifier to ballot
number plus the screening order), named ballot streams, and run_stream, which
casts a stream into a box and checks every result, the tally, the state, the
log and the recount against the model.  Shared by the host-path and the
device-path tests; the model is the oracle for both.

Home-slot rule the crafted streams rely on (csrc/ballot_table.h): a box of
capacity C has S = the power of two >= 2 C slots, and a nullifier's home slot
is nullifier[0] & (S - 1); the probe goes to the next slot, wrapping."""
import random

import numpy as np

P = 0xFFFFFFFF00000001
PROPOSAL = [0x2A2A2A2A2A2A2A2A, 1, 2, 3]
OTHER_PROPOSAL = [0x2A2A2A2A2A2A2A2A, 1, 2, 4]
ROOT_A = [11, 12, 13, P - 1]
ROOT_B = [21, 22, 23, 24]
ROOT_UNKNOWN = [11, 12, 13, P - 2]

COUNTED, PROOF_REJECTED, MALFORMED, WRONG_PROPOSAL, UNKNOWN_ROOT, BAD_VOTE, DOUBLE_VOTE = range(7)
BATCHINGS = [1, 7, 64, None]  # None: every run of ballots between two reserves as one batch


class Model:
    def __init__(self, proposal, roots):
        self.proposal, self.roots = list(proposal), [list(r) for r in roots]
        self.seen, self.log, self.cast, self.yes, self.no = {}, [], 0, 0, 0

    def screen(self, pi, verdict):
        if verdict:
            return PROOF_REJECTED
        if len(pi) != 13 or any(not 0 <= x < P for x in pi):
            return MALFORMED
        if pi[0:4] != self.proposal:
            return WRONG_PROPOSAL
        if pi[4:8] not in self.roots:
            return UNKNOWN_ROOT
        if pi[8] not in (0, 1):
            return BAD_VOTE
        return COUNTED

    def cast_one(self, pi, verdict):
        """(status, verify_status, number, first)"""
        num, self.cast = self.cast, self.cast + 1
        st = self.screen(pi, verdict)
        if st:
            return (st, verdict, num, num)
        nul = tuple(pi[9:13])
        first = self.seen.setdefault(nul, num)
        self.log.append((nul, num, first == num, bool(pi[8])))
        if first != num:
            return (DOUBLE_VOTE, verdict, num, first)
        self.yes, self.no = self.yes + pi[8], self.no + 1 - pi[8]
        return (COUNTED, verdict, num, num)


def ballot(nullifier, vote=1, proposal=PROPOSAL, root=ROOT_A):
    return list(proposal) + list(root) + [vote] + list(nullifier)


def _nullifiers(rng, n):
    return [[rng.randrange(P) for _ in range(4)] for _ in range(n)]


def _homed(rng, home, slots):
    """a felt 0 whose home slot in a table of `slots` slots is `home`"""
    return (rng.randrange(1 << 40) * slots) | home


def make_stream(name):
    """(capacity, roots, items): an item is (public inputs, verdict) or ("reserve", capacity)"""
    rng = random.Random("ballot " + name)
    vote = lambda: rng.randrange(2)  # noqa: E731
    roots = [ROOT_A]
    if name == "distinct":
        cap, items = 32, [(ballot(n, vote()), 0) for n in _nullifiers(rng, 32)]
    elif name == "one_nullifier":
        n = _nullifiers(rng, 1)[0]
        cap, items = 64, [(ballot(n, vote()), 0) for _ in range(64)]
    elif name == "across_batches":
        first = [(ballot(n, vote()), 0) for n in _nullifiers(rng, 32)]
        cap, items = 64, first + [(ballot(pi[9:13], 1 - pi[8]), 0) for pi, _ in first]
    elif name == "chain_wrap":
        cap, slots = 64, 128
        f0 = _homed(rng, slots - 2, slots)
        nuls = [[f0, 1000 + i, 7, 7] for i in range(20)]
        cap, items = 64, [(ballot(n, vote()), 0) for n in nuls + nuls]
    elif name == "felt3_only":
        base = _nullifiers(rng, 1)[0][:3]
        cap, items = 16, [(ballot(base + [i], vote()), 0) for i in range(16)]
    elif name == "two_keys_shuffled":
        cap, slots = 64, 128
        a, b = [[_homed(rng, 5, slots), 1, 2, 3] for _ in range(2)]
        assert a != b
        order = [a] * 30 + [b] * 30
        rng.shuffle(order)
        items = [(ballot(n, vote()), 0) for n in order]
    elif name == "many_blocks":
        order = _nullifiers(rng, 2048) * 4
        rng.shuffle(order)
        cap, items = 8192, [(ballot(n, vote()), 0) for n in order]
    elif name == "screened":
        roots = [ROOT_A, ROOT_B]
        g = _nullifiers(rng, 8)
        cap, items = 16, [
            (ballot(g[0], 1), 0),
            (ballot(g[1], 1, proposal=OTHER_PROPOSAL), 0),
            (ballot(g[1], 0, root=ROOT_B), 0),
            (ballot(g[2], 1, root=ROOT_UNKNOWN), 0),
            (ballot(g[2], 2), 0),
            (ballot(g[2][:3] + [P], 1), 0),
            (ballot(g[2], 1), 9),                                        # the verifier's "malformed" verdict
            (ballot(g[2], 1), 0),
            (ballot(g[3], 2, proposal=OTHER_PROPOSAL, root=ROOT_UNKNOWN), 0),  # three failures: the first names it
            (ballot(g[3], 2, root=ROOT_UNKNOWN), 0),                     # two: the root's comes before the vote's
            (ballot(g[3], P, proposal=OTHER_PROPOSAL), 3),               # rejected proof before anything else
            (ballot(g[3], P, proposal=OTHER_PROPOSAL), 0),               # malformed before wrong proposal
            (ballot(g[0], 0), 0),                                        # a double of the first ballot
            (ballot(g[3], 0)[:12], 0),                                   # 12 public inputs
            (ballot(g[3], 0), 0),
            (ballot(g[1], 1), 0),                                        # a double under another accepted root
        ]
    elif name == "grow":
        g = _nullifiers(rng, 100)
        b = lambda i: (ballot(g[i], vote()), 0)  # noqa: E731
        items = ([b(i) for i in range(24)] + [b(3), b(3)] + [("reserve", 64)] +
                 [b(i) for i in (0, 23, 24, 25, 5)] + [b(i) for i in range(26, 50)] + [("reserve", 128)] +
                 [b(i) for i in (1, 24, 49, 50)] + [b(i) for i in range(51, 100)] + [b(99), b(0)])
        cap = 32
    else:
        raise KeyError(name)
    return cap, roots, items


STREAMS = ["distinct", "one_nullifier", "across_batches", "chain_wrap", "felt3_only", "two_keys_shuffled",
           "many_blocks", "screened", "grow"]


def batches(items, batching):
    """the stream as ("cast", [items]) and ("reserve", capacity) steps"""
    run = []
    for it in list(items) + [("reserve", None)]:
        if it[0] == "reserve":
            step = batching or max(len(run), 1)
            for at in range(0, len(run), step):
                yield "cast", run[at:at + step]
            run = []
            if it[1] is not None:
                yield it
        else:
            run.append(it)


def cast_batch(box, batch):
    rows = [pi for pi, _ in batch]
    verdicts = [v for _, v in batch]
    pis = np.array(rows, dtype=np.uint64) if all(len(r) == 13 for r in rows) else rows
    return box.cast_public(pis, verdicts if any(verdicts) else None, reserve=False)


def run_stream(box_factory, name, batching):
    """Casts stream `name` cut into batches of `batching` into box_factory(PROPOSAL,
    roots, capacity), checks everything observable against the model and returns
    the results (tuples), for comparison across batchings and paths."""
    cap, roots, items = make_stream(name)
    model = Model(PROPOSAL, roots)
    box = box_factory(PROPOSAL, roots, cap)
    results = []
    try:
        for kind, arg in batches(items, batching):
            if kind == "reserve":
                box.reserve(arg)
                cap = arg
                continue
            got = [tuple(r) for r in cast_batch(box, arg)]
            want = [model.cast_one(pi, v) for pi, v in arg]
            assert got == want, (name, batching, len(results))
            results += got
        assert box.tally == (model.yes, model.no)
        assert (box.cast_count, box.admitted, box.capacity) == (model.cast, len(model.log), cap)
        nul, num, counted, votes = box.entries()
        assert [tuple(int(x) for x in r) for r in nul] == [e[0] for e in model.log]
        assert [int(x) for x in num] == [e[1] for e in model.log]
        assert [bool(x) for x in counted] == [e[2] for e in model.log]
        assert [bool(x) for x in votes] == [e[3] for e in model.log]
        assert box.recount() == (model.yes, model.no, model.yes + model.no, len(model.log))
        if len(model.log) > 3:  # a window of the log
            n2, m2, c2, v2 = box.entries(1, 2)
            assert (n2 == nul[1:3]).all() and (m2 == num[1:3]).all() and (c2 == counted[1:3]).all()
    finally:
        box.free()
    return results
