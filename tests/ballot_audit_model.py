"""The audit of a published ballot log as a model, pure Python over
ballot_model.Model.log and the tree functions of ballot_receipt_model.py, and
the cases the host-path and the device tests both run.  The model is the oracle
of both paths; nothing in it calls the code under test.

Definitions (include/qpgpu.h, csrc/ballot_audit.h).  A published
log is nullifiers[n][4], numbers[n], flags[n] (bit 0 the vote, bit 1 counted);
beside it come optional claims: a root, a tally (yes, no), earlier commitments
(root_i, n_i).  The audit reports the first reason that fires, in this order,
with the lowest offender as its witness:
  1 NON_CANONICAL a felt >= p, a number >= p or flags > 3: the lowest such seq;
                  root and counts are zero
  2 ORDER         numbers[seq] <= numbers[seq - 1]: the lowest such seq >= 1
  3 COUNT_RULE    counted bit != "no earlier entry has this nullifier": the
                  lowest such seq, first = the lowest seq with that nullifier
  4 TALLY         a claimed tally != (counted & vote, counted & !vote)
  5 ROOT          a claimed root != the root over [0, n)
  6 COMMITMENT    n_i > n or prefix_root(n_i) != root_i: the lowest such i
prefix_root(m) is the root of the tree over leaves [0, m):
tree_from_leaves(leaves[:m]).  Logs above 300 entries take it from LogModel's
kept full nodes instead (the same recursion the receipt tests hold equal to
tree_from_leaves) and hold the two equal at a few m.
"""
from collections import namedtuple

import numpy as np

from ballot_model import PROPOSAL, ROOT_A, Model, ballot, batches, cast_batch, make_stream
from ballot_receipt_model import LogModel
from oracle_lib import P, hash_no_pad
from registry_open_model import tree_from_leaves

OK, NON_CANONICAL, ORDER, COUNT_RULE, TALLY, ROOT, COMMITMENT = range(7)
SIZES = [1, 2, 3, 5, 64, 65, 131, 257]
Report = namedtuple("Report", "status witness first root yes no counted")


def log_of(entries):
    """[(nullifier tuple, number, flags byte)] from a box's entries() 4-tuple or (nullifiers, numbers, flags)"""
    if len(entries) == 4:
        nul, num, counted, votes = entries
        fl = [int(v) | int(c) << 1 for c, v in zip(counted, votes)]
    else:
        nul, num, fl = entries
    return [(tuple(int(x) for x in k), int(m), int(f)) for k, m, f in zip(nul, num, fl)]


def arrays_of(log):
    """(nullifiers, numbers, flags) arrays of a model log, the 3-tuple audit_log takes"""
    return (np.array([e[0] for e in log], dtype=np.uint64).reshape(len(log), 4),
            np.array([e[1] for e in log], dtype=np.uint64), np.array([e[2] for e in log], dtype=np.uint8))


class Tree:
    """prefix roots of one canonical log"""

    def __init__(self, log):
        self.leaves = [hash_no_pad(list(k) + [m, f]) for k, m, f in log]
        self.kept = {}
        self.fast = None
        if len(log) > 300:
            self.fast = LogModel()
            self.fast.leaves = self.leaves

    def prefix_root(self, m):
        assert 1 <= m <= len(self.leaves)
        if m not in self.kept:
            n = len(self.leaves)
            if self.fast is None or m in (1, 2, 257, n // 2 + 1, n - 1, n):
                self.kept[m] = tree_from_leaves(self.leaves[:m])[-1][0]
                assert self.fast is None or self.fast.root(m) == self.kept[m]
            else:
                self.kept[m] = self.fast.root(m)
        return self.kept[m]


def audit(log, root=None, tally=None, commitments=()):
    """the model's verdict on `log` ([(nullifier, number, flags)]) and the claims"""
    n = len(log)
    assert 1 <= n <= 1 << 31 and all(c[1] >= 1 for c in commitments)
    for seq, (nul, num, fl) in enumerate(log):
        if any(x >= P for x in nul) or num >= P or fl > 3:
            return Report(NON_CANONICAL, seq, None, [0, 0, 0, 0], 0, 0, 0)
    order = next((seq for seq in range(1, n) if log[seq][1] <= log[seq - 1][1]), None)
    seen, rule = {}, None
    for seq, (nul, num, fl) in enumerate(log):
        first = seen.setdefault(nul, seq)
        if bool(fl & 2) != (first == seq) and rule is None:
            rule = (seq, first)
    yes = sum(1 for e in log if e[2] == 3)
    no = sum(1 for e in log if e[2] == 2)
    tree = Tree(log)
    got = tree.prefix_root(n)
    rest = (got, yes, no, yes + no)
    if order is not None:
        return Report(ORDER, order, None, *rest)
    if rule is not None:
        return Report(COUNT_RULE, rule[0], rule[1], *rest)
    if tally is not None and tuple(tally) != (yes, no):
        return Report(TALLY, None, None, *rest)
    if root is not None and list(root) != got:
        return Report(ROOT, None, None, *rest)
    for i, (r_i, n_i) in enumerate(commitments):
        if n_i > n or tree.prefix_root(n_i) != list(r_i):
            return Report(COMMITMENT, i, None, *rest)
    return Report(OK, None, None, *rest)


def same(rep, want):
    """an AuditReport of the code under test against the model's Report, field for field"""
    assert tuple(rep) == tuple(want), (tuple(rep), tuple(want))
    return tuple(rep)


# ---- the cases both paths run.  ctx: a Context or None, what audit_log and restore run on;
# box_factory(proposal, roots, capacity) makes the boxes of the same path.

def check_honest_stream(ctx, box_factory, name):
    """stream `name` through a real box in batches of 7, a commitment taken after
    every batch; the log audited with its own (root, n, tally) and all of them"""
    from qp_wormhole import audit_log
    cap, roots, items = make_stream(name)
    box = box_factory(PROPOSAL, roots, cap)
    commitments = []
    try:
        for kind, arg in batches(items, 7):
            if kind == "reserve":
                box.reserve(arg)
                continue
            cast_batch(box, arg)
            if box.admitted:
                commitments.append(box.commit_log())
        root, n = box.commit_log()
        entries, tally = box.entries(), box.tally
    finally:
        box.free()
    assert n == len(entries[1]) and commitments[-1] == (root, n)
    rep = audit_log(ctx, entries, root=root, tally=tally, commitments=commitments)
    assert (rep.status, rep.witness, rep.first) == (OK, None, None)
    assert (rep.root, (rep.yes, rep.no), rep.counted) == (root, tally, sum(tally))
    return same(rep, audit(log_of(entries), root, tally, commitments))


def distinct_items(n, seed=None):
    rng = np.random.default_rng(n if seed is None else seed)
    nuls = rng.integers(0, P, size=(n, 4), dtype=np.uint64).tolist()
    return [(ballot(k, i & 1), 0) for i, k in enumerate(nuls)]


def check_size(ctx, box_factory, n):
    """n distinct admitted ballots in a box of exactly that capacity: the audit of
    its log with the root, the tally and the commitments at 1, n // 2 + 1 and n"""
    from qp_wormhole import audit_log
    box = box_factory(PROPOSAL, [ROOT_A], n)
    try:
        cast_batch(box, distinct_items(n))
        root, got_n = box.commit_log()
        entries, tally = box.entries(), box.tally
        ms = sorted({1, n // 2 + 1, n})
        commitments = list(zip(box.roots_at(ms), ms))
    finally:
        box.free()
    assert got_n == n
    rep = audit_log(ctx, entries, root=root, tally=tally, commitments=commitments)
    assert rep.status == OK and rep.root == root
    return same(rep, audit(log_of(entries), root, tally, commitments))


def check_roots_at_every_m(box_factory, n=131):
    """n ballots cast one at a time, the log committed at every size: roots_at of
    every m equals the root the box reported at that size, and the model's"""
    box = box_factory(PROPOSAL, [ROOT_A], n)
    try:
        reported = []
        for it in distinct_items(n):
            cast_batch(box, [it])
            reported.append(box.commit_log())
        assert [m for _, m in reported] == list(range(1, n + 1))
        got = box.roots_at(range(1, n + 1))
        assert got == [r for r, _ in reported]
        tree = Tree(log_of(box.entries()))
        assert got == [tree.prefix_root(m) for m in range(1, n + 1)]
        assert box.root_at(n) == box.commit_log()[0] and box.root_at(1) == tree.leaves[0]
        assert box.roots_at([]) == [] and box.roots_at([n, 1, n]) == [got[-1], got[0], got[-1]]
        return got
    finally:
        box.free()


# the tampering base: 700 entries, three blocks of 256 lanes.  Doubles: 20 of 10 (one wave), 600 of
# 5 (different blocks), 300 of 299 (neighbours)
BASE_N, DOUBLES = 700, {20: 10, 600: 5, 300: 299}
BASE_MS = [100, 400, 650]


def base_log(box_factory):
    """(log, root, tally, commitments at BASE_MS) of the honest base, through a real box"""
    items = distinct_items(BASE_N, seed=77)
    for d, first in DOUBLES.items():
        items[d] = (ballot(items[first][0][9:13], 1 - items[first][0][8]), 0)
    box = box_factory(PROPOSAL, [ROOT_A], BASE_N)
    try:
        cast_batch(box, items)
        root, n = box.commit_log()
        log, tally = log_of(box.entries()), box.tally
        commitments = list(zip(box.roots_at(BASE_MS), BASE_MS))
    finally:
        box.free()
    assert n == BASE_N and [s for s, e in enumerate(log) if not e[2] & 2] == sorted(DOUBLES)
    return log, root, tally, commitments


def _edit(log, **at):
    """a copy of log with entries replaced: _edit(log, s20=lambda k, m, f: (k, m, f | 2))"""
    out = list(log)
    for key, fn in at.items():
        s = int(key[1:])
        out[s] = fn(*out[s])
    return out


def _swap_numbers(log, a, b):
    out = list(log)
    out[a], out[b] = (log[a][0], log[b][1], log[a][2]), (log[b][0], log[a][1], log[b][2])
    return out


def tamperings(log, root, tally, commitments):
    """[(what, log, claims, (status, witness, first))]: each tampering alone, two of
    one reason, two of two reasons.  claims = (root, tally, commitments)."""
    everything = (root, tally, commitments)
    set_counted = lambda k, m, f: (k, m, f | 2)  # noqa: E731
    flip_vote = lambda k, m, f: (k, m, f ^ 1)  # noqa: E731
    felt_p = lambda k, m, f: (k[:2] + (P,) + k[3:], m, f)  # noqa: E731
    assert log[7][2] & 2 and not log[300][2] & 2
    rewritten = _edit(log, s300=flip_vote)  # a double's vote: the tally stays, every root from 301 entries on moves
    cheat_root = Tree(rewritten).prefix_root(len(log))
    return [
        ("felt = p", _edit(log, s650=felt_p), everything, (NON_CANONICAL, 650, None)),
        ("number = p", _edit(log, s3=lambda k, m, f: (k, P, f)), everything, (NON_CANONICAL, 3, None)),
        ("flags = 4", _edit(log, s256=lambda k, m, f: (k, m, 4)), everything, (NON_CANONICAL, 256, None)),
        ("numbers swapped over a block edge", _swap_numbers(log, 255, 256), everything, (ORDER, 256, None)),
        ("numbers equal", _edit(log, s40=lambda k, m, f: (k, log[39][1], f)), everything, (ORDER, 40, None)),
        ("first ballot not counted", _edit(log, s10=lambda k, m, f: (k, m, f & 1)), everything, (COUNT_RULE, 10, 10)),
        ("double counted, one wave", _edit(log, s20=set_counted), everything, (COUNT_RULE, 20, 10)),
        ("double counted, other block", _edit(log, s600=set_counted), everything, (COUNT_RULE, 600, 5)),
        ("vote flipped, old tally", _edit(log, s7=flip_vote), (None, tally, ()), (TALLY, None, None)),
        ("vote flipped, old root", _edit(log, s7=flip_vote), (root, None, ()), (ROOT, None, None)),
        ("history rewritten", rewritten, (cheat_root, tally, commitments), (COMMITMENT, 1, None)),
        ("n_i > n", log, (root, tally, commitments[:1] + [(root, len(log) + 1)]), (COMMITMENT, 1, None)),
        ("two counted doubles in two blocks", _edit(log, s600=set_counted, s20=set_counted), everything,
         (COUNT_RULE, 20, 10)),
        ("two non-canonical in two blocks", _edit(log, s650=felt_p, s3=felt_p), everything, (NON_CANONICAL, 3, None)),
        ("two swaps in two blocks", _swap_numbers(_swap_numbers(log, 610, 611), 30, 31), everything, (ORDER, 31, None)),
        ("order and count rule", _edit(_swap_numbers(log, 500, 501), s20=set_counted), everything, (ORDER, 501, None)),
        ("non-canonical and order", _edit(_swap_numbers(log, 39, 40), s650=felt_p), everything,
         (NON_CANONICAL, 650, None)),
        ("count rule, tally and root", _edit(log, s20=set_counted), everything, (COUNT_RULE, 20, 10)),
        ("tally and root", _edit(log, s7=flip_vote), everything, (TALLY, None, None)),
        ("root and commitment", _edit(log, s300=flip_vote), everything, (ROOT, None, None)),
    ]


def check_tamperings(ctx, box_factory):
    from qp_wormhole import audit_log
    log, root, tally, commitments = base_log(box_factory)
    honest = audit_log(ctx, arrays_of(log), root=root, tally=tally, commitments=commitments)
    out = [same(honest, audit(log, root, tally, commitments))]
    assert honest.status == OK
    for what, bad, (r, t, cs), want in tamperings(log, root, tally, commitments):
        before = [a.copy() for a in arrays_of(bad)]
        arrays = [a.copy() for a in before]
        rep = audit_log(ctx, tuple(arrays), root=r, tally=t, commitments=cs)
        assert (rep.status, rep.witness, rep.first) == want, what
        assert all((a == b).all() for a, b in zip(arrays, before)), what  # an audit never alters what it was given
        out.append(same(rep, audit(bad, r, t, cs)))
    return out


REPLAY_STRIDE = 97


def restore_cuts(name, every_cut=True):
    """(steps, cuts, replayed) of stream `name` under batching 7: a restore is
    tried, and held to the uninterrupted box's state at that point, after every
    cast step in `cuts`; after those in `replayed` the restored box also casts
    the rest of the stream.  A stream of at most 40 batches is replayed from
    every cut.  A longer one (many_blocks: 1171 batches) is restored and
    checked at every cut, and replayed from the first three, the last three and
    every 97th, since each replay costs the rest of the stream.  every_cut =
    False keeps only the replayed cuts of a long stream: for callers that say
    why they subsample."""
    steps = list(batches(make_stream(name)[2], 7))
    casts = [i for i, s in enumerate(steps) if s[0] == "cast"]
    if len(casts) <= 40:
        return steps, casts, set(casts)
    replayed = set(casts[:3] + casts[-3:] + casts[::REPLAY_STRIDE])
    return steps, (casts if every_cut else sorted(replayed)), replayed


def observe(box, model_nullifiers):
    """everything observable of a box after its stream"""
    from qp_wormhole import BallotBox
    nul, num, counted, votes = box.entries()
    out = [nul.tolist(), num.tolist(), counted.tolist(), votes.tolist(), box.tally, box.cast_count, box.admitted]
    if box.admitted:
        out.append(box.commit_log())
        out.append(box.find(model_nullifiers))
        r = box.receipts([box.admitted - 1])[0]
        assert BallotBox.check_receipt(r)
        out.append(tuple(r))
    return out


def check_restore_stream(ctx, box_factory, name, entries_factory=None, every_cut=True):
    """For each cut (restore_cuts): a box restored from the entries at the cut,
    with the root the log had there expected, has the uninterrupted box's state,
    tally, commitment and `find` answers of that point, and a receipt of its last
    entry checks.  From the replayed cuts it then casts the rest of the stream
    (each run between reserves as one batch); results and everything observable
    equal the uninterrupted box's.  entries_factory: the path whose box
    publishes the entries (default: box_factory's)."""
    from qp_wormhole import BallotBox
    from qp_wormhole.ballot import NOT_FOUND
    cap0, roots, items = make_stream(name)
    steps, cuts, replayed = restore_cuts(name, every_cut)
    # the uninterrupted box, and what it had published after each step
    box = (entries_factory or box_factory)(PROPOSAL, roots, cap0)
    results, state, cap = [], [], cap0
    try:
        for kind, arg in steps:
            if kind == "reserve":
                box.reserve(arg)
                cap = arg
            else:
                results += [tuple(r) for r in cast_batch(box, arg)]
            state.append((box.admitted, box.cast_count, cap, len(results), box.tally))
        nullifiers = [list(k) for k in dict.fromkeys(tuple(pi[9:13]) for pi, _ in items if len(pi) == 13
                                                      and all(0 <= x < P for x in pi[9:13]))]
        queries = np.array(nullifiers, dtype=np.uint64)
        final_entries = box.entries()
        want = observe(box, nullifiers)
        # the counted entry of a nullifier is its lowest seq, so at a cut `find` answers the final seq or nothing
        final_find = box.find(queries, raw=True)
        prefix_roots = box.roots_at([s[0] for s in state if s[0]]) if box.admitted else []
    finally:
        box.free()
    at_root = dict(zip([s[0] for s in state if s[0]], prefix_roots))
    for c in cuts:
        admitted, cast_count, cap, done, tally = state[c]
        entries = tuple(a[:admitted] for a in final_entries)
        again = BallotBox.restore(ctx, PROPOSAL, roots, entries, cast_count=cast_count, capacity=cap,
                                  root=at_root.get(admitted))
        try:
            assert (again.admitted, again.cast_count, again.capacity, again.tally) == (admitted, cast_count, cap, tally)
            if admitted:
                assert again.commit_log() == (at_root[admitted], admitted), (name, c)
                found = again.find(queries, raw=True)
                assert (found == np.where(final_find < admitted, final_find, np.uint64(NOT_FOUND))).all(), (name, c)
                r = again.receipts([admitted - 1])[0]
                assert BallotBox.check_receipt(r) and (r.root, r.n) == (at_root[admitted], admitted), (name, c)
            if c not in replayed:
                continue
            rest = [it for s in steps[c + 1:] for it in (s[1] if s[0] == "cast" else [s])]
            got = []
            for kind, arg in batches(rest, None):
                if kind == "reserve":
                    again.reserve(arg)
                else:
                    got += [tuple(r) for r in cast_batch(again, arg)]
            assert got == results[done:], (name, c)
            assert observe(again, nullifiers) == want, (name, c)
        finally:
            again.free()
    return want


def check_restore_refusals(ctx, box_factory):
    import pytest
    from qp_wormhole import BallotBox, QpError
    log, root, tally, commitments = base_log(box_factory)

    def restore(bad, **kw):
        box = BallotBox.restore(ctx, PROPOSAL, [ROOT_A], arrays_of(bad), **kw)
        box.free()

    restore(log, root=root)
    restore(log, capacity=BASE_N, cast_count=log[-1][1] + 1)
    for what, bad, _, (status, witness, first) in tamperings(log, root, tally, commitments)[:8]:
        reason = {NON_CANONICAL: "non-canonical", ORDER: "out of order", COUNT_RULE: "count rule"}[status]
        with pytest.raises(QpError, match=f"QP_ERR_FORMAT.*{reason}.*entry {witness}\\b"):
            restore(bad)
    with pytest.raises(QpError, match="QP_ERR_FORMAT.*count rule.*entry 600, its nullifier first at entry 5\\b"):
        restore(_edit(log, s600=lambda k, m, f: (k, m, f | 2)))
    with pytest.raises(QpError, match="QP_ERR_FORMAT.*claimed root differs"):
        restore(_edit(log, s7=lambda k, m, f: (k, m, f ^ 1)), root=root)
    restore(_edit(log, s7=lambda k, m, f: (k, m, f ^ 1)))  # no root expected: a restore takes the tally from the flags
    with pytest.raises(QpError, match="QP_ERR_ARG.*cast_count"):
        restore(log, cast_count=log[-1][1])
    with pytest.raises(QpError, match="QP_ERR_ARG.*capacity"):
        restore(log, capacity=BASE_N - 1)
    empty = BallotBox.restore(ctx, PROPOSAL, [ROOT_A], arrays_of([]), cast_count=5, capacity=4)
    try:
        assert (empty.admitted, empty.cast_count, empty.tally) == (0, 5, (0, 0))
        res = cast_batch(empty, distinct_items(2))
        assert [(r.status, r.number) for r in res] == [(0, 5), (0, 6)]
    finally:
        empty.free()
