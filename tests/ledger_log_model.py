"""The transfer ledger's log commitment and the audit of a published transfer
log as a model, from ledger_model.Model and the oracle's hash_no_pad alone,
and the cases the host-path and the device tests both run.  Nothing in the
model calls the code under test.

Definitions (include/qpgpu.h).  Log leaf of entry seq =
hash_no_pad([nullifier[0..4], number, amount[0..4], account[0..4], flags]): 14
felts, the amount as its four 32-bit limbs most significant first, flags bit 0
= credited.  The tree over leaves [0, n) in the registry's convention
(registry_open_model.tree_from_leaves, paths by registry_oracle.oracle_path,
through ballot_receipt_model.LogModel, which only hashes and caches nodes); the
commitment is (root, n); the shape rule of a path is ballot_receipt_model.shape.

The audit reports the first reason that fires, in this order, with the lowest
offender as its witness:
  1 NON_CANONICAL a nullifier or account felt >= p, a number >= p or flags > 1
  2 ORDER         numbers[seq] <= numbers[seq - 1]
  3 CREDIT_RULE   credited bit != "no earlier entry has this nullifier"; first
                  = the lowest seq with that nullifier
  4 TOTALS        claimed (credited, total) != the log's
  5 PAYOUTS       the claimed list != the log's payouts in first-credit order:
                  the lowest i < min(A, K) that differs, else A != K: min(A, K)
  6 ROOT          claimed root != the root over [0, n)
  7 COMMITMENT    n_i > n or the prefix root at n_i != root_i: the lowest i
"""
import ctypes
from collections import namedtuple

import numpy as np

from ballot_receipt_model import LogModel, shape
from ledger_model import MAX_AMOUNT, ROOT_A, Model, batches, cast_batch, limbs_of, make_stream, transfer
from oracle_lib import P, hash_no_pad
from registry_open_model import tree_from_leaves

SIZES = [1, 2, 3, 5, 65, 131]
OK, NON_CANONICAL, ORDER, CREDIT_RULE, TOTALS, PAYOUTS, ROOT, COMMITMENT = range(8)
Report = namedtuple("Report", "status witness first root credited total accounts")


def felts_of(entry):
    """the 14 felts of a model log entry (nullifier, number, amount int, account, credited)"""
    nul, num, amount, acc, credited = entry
    return list(nul) + [num] + limbs_of(amount) + list(acc) + [int(credited)]


def leaf(entry):
    return hash_no_pad(felts_of(entry))


class LedgerLogModel(LogModel):
    """LogModel (the tree over kept leaves, root(n), path(seq, n)) with the ledger's leaf"""

    def sync(self, model):
        for e in model.log[len(self.leaves):]:
            self.leaves.append(leaf(e))


def check_receipt(r, root=None, n=None):
    """the receipt check in pure Python over the oracle's hash"""
    root = list(r.root if root is None else root)
    n = r.n if n is None else n
    felts = list(root) + list(r.nullifier) + [r.number] + list(r.account) + [x for s in r.siblings for x in s]
    if any(not 0 <= x < P for x in felts) or len(r.amount) != 4 or any(not 0 <= x < 1 << 32 for x in r.amount):
        return False
    if not 1 <= n <= 1 << 31 or not 0 <= r.seq < n:
        return False
    if (r.depth, r.path_bits) != shape(r.seq, n) or len(r.siblings) != r.depth:
        return False
    cur = hash_no_pad(list(r.nullifier) + [r.number] + list(r.amount) + list(r.account) + [int(bool(r.credited))])
    for j, s in enumerate(r.siblings):
        cur = hash_no_pad(list(s) + cur if r.path_bits >> j & 1 else cur + list(s))
    return cur == root


def assert_receipt(r, model, logm, n):
    """receipt r of entry r.seq under n entries equals the model's, and both checkers accept it"""
    from qp_wormhole import WormholeLedger
    nul, num, amount, acc, credited = model.log[r.seq]
    sibs, bits, depth = logm.path(r.seq, n)
    assert (tuple(r.nullifier), r.number, r.amount, tuple(r.account), r.credited) == \
        (nul, num, limbs_of(amount), acc, credited), r.seq
    assert r.total == amount
    assert (r.siblings, r.path_bits, r.depth) == (sibs, bits, depth), (r.seq, n)
    assert (r.root, r.n) == (logm.root(n), n)
    assert check_receipt(r) and WormholeLedger.check_receipt(r), (r.seq, n)


# ---- the commitment cases both paths run (ledger_factory(roots, padding, capacity) makes the ledger)

def run_commit_stream(ledger_factory, name, batching, every_batch=True):
    """Casts stream `name` in batches of `batching`; with every_batch commits after
    each batch (and around each reserve) and holds the root to the model's at that
    n, else commits once at the end.  Returns (root, n, receipts of the first, a
    middle and the last entry); (None, 0, []) for a stream that admits nothing."""
    from qp_wormhole import QpError
    cap, roots, padding, items = make_stream(name)
    model, logm = Model(roots, padding), LedgerLogModel()
    led = ledger_factory(roots, padding, cap)
    try:
        for kind, arg in batches(items, batching):
            if kind == "reserve":
                before = led.commit_log() if every_batch and model.log else None
                led.reserve(arg)
                if before is not None:
                    n = len(model.log)
                    assert led.commit_log() == before == (logm.root(n), n)  # a reserve leaves the root unchanged
                    for r in led.receipts(sorted({0, n - 1, n // 2})):
                        assert_receipt(r, model, logm, n)
                continue
            cast_batch(led, arg)
            for pi, v in arg:
                model.cast_one(pi, v)
            logm.sync(model)
            if every_batch and model.log:
                n = len(model.log)
                assert led.commit_log() == (logm.root(n), n), (name, batching, n)
        n = len(model.log)
        if not n:
            try:
                led.commit_log()
            except QpError as e:
                assert "QP_ERR_STATE" in str(e) and "empty log" in str(e)
                return None, 0, []
            raise AssertionError("an empty log was committed")
        root, got_n = led.commit_log()
        assert (root, got_n) == (logm.root(n), n), (name, batching)
        assert root == logm.tree(n)[-1][0]  # the level loop from scratch
        assert (led.log_root, led.log_size) == (root, n)
        rs = led.receipts(sorted({0, n // 2, n - 1}))
        for r in rs:
            assert_receipt(r, model, logm, n)
        return root, n, [tuple(r) for r in rs]
    finally:
        led.free()


def sized_items(n, seed=None, accounts=5):
    """n transfers with distinct nullifiers to `accounts` accounts, random amounts"""
    rng = np.random.default_rng(n if seed is None else seed)
    nuls = rng.integers(0, P, size=(n, 4), dtype=np.uint64).tolist()
    accs = rng.integers(0, P, size=(accounts, 4), dtype=np.uint64).tolist()
    amts = [int.from_bytes(rng.bytes(16), "little") for _ in range(n)]
    return [(transfer(k, amts[i], accs[i % accounts]), 0) for i, k in enumerate(nuls)]


def sized_ledger(ledger_factory, items, capacity=None):
    model, logm = Model([ROOT_A]), LedgerLogModel()
    led = ledger_factory([ROOT_A], None, capacity or len(items))
    try:
        cast_batch(led, items)
    except BaseException:
        led.free()
        raise
    for pi, v in items:
        model.cast_one(pi, v)
    logm.sync(model)
    return led, model, logm


def check_size(ledger_factory, n):
    """n admitted entries in a ledger of exactly that capacity: the root, and the
    receipts of seq 0, n - 1 and n - 2 against the model's paths"""
    led, model, logm = sized_ledger(ledger_factory, sized_items(n))
    try:
        assert led.commit_log() == (logm.root(n), n) and logm.root(n) == logm.tree(n)[-1][0]
        seqs = sorted({0, n - 1, max(n - 2, 0)})
        rs = led.receipts(seqs)
        assert [r.seq for r in rs] == seqs
        for r in rs:
            assert_receipt(r, model, logm, n)
        got = led.entries_at(seqs[::-1])
        assert [tuple(int(x) for x in k) for k in got[0]] == [model.log[s][0] for s in seqs[::-1]]
        assert got[2] == [model.log[s][2] for s in seqs[::-1]]
        return [tuple(r) for r in rs]
    finally:
        led.free()


def edge_items():
    """transfers whose leaves carry the edge values: amount limbs 0 and 2^32 - 1 in every position,
    account and nullifier felts 0 and p - 1, and a double spend (flags 0) as the last entry"""
    items, top = [], 0xFFFFFFFF
    for pos in range(4):
        for limbs in ([top if j == pos else 0 for j in range(4)], [0 if j == pos else top for j in range(4)]):
            items.append((transfer([100 + len(items), 1, 2, 3], limbs=limbs, account=[7, 7, 7, len(items)]), 0))
    items.append((transfer([200, 0, 0, 0], limbs=[0] * 4, account=[0, 0, 0, 0]), 0))
    items.append((transfer([0, 0, 0, 0], limbs=[top] * 4, account=[P - 1] * 4), 0))
    items.append((transfer([P - 1] * 4, 5, [0, P - 1, 0, P - 1]), 0))
    items.append((transfer([P - 1, 0, P - 1, 0], MAX_AMOUNT, [P - 1, 0, 0, 0]), 0))
    items.append((transfer([0, 0, 0, 0], 9, [1, 2, 3, 4]), 0))  # a double spend of [0, 0, 0, 0]
    return items


def check_leaf_edges(ledger_factory):
    """every edge entry's leaf, as the library's receipts report it, equals the oracle's hash of the 14
    felts and the library's own qp_hash_no_pad of them"""
    from qp_wormhole._native import hash_no_pad as lib_hash, lib
    items = edge_items()
    led, model, logm = sized_ledger(ledger_factory, items)
    try:
        k = len(items)
        assert [e[4] for e in model.log] == [True] * (k - 1) + [False]
        seqs = np.arange(k, dtype=np.uint64)
        sib = np.zeros((k, 32, 4), np.uint64)
        bits, depth = np.zeros(k, np.uint32), np.zeros(k, np.uint32)
        leaves, root, n = np.zeros((k, 4), np.uint64), np.zeros(4, np.uint64), ctypes.c_uint64()
        assert lib().qp_ledger_receipts(led.h, seqs.ctypes.data, k, sib.ctypes.data, bits.ctypes.data,
                                        depth.ctypes.data, leaves.ctypes.data, root.ctypes.data, ctypes.byref(n)) == 0
        for i, e in enumerate(model.log):
            felts = felts_of(e)
            assert len(felts) == 14
            assert leaves[i].tolist() == leaf(e) == [int(x) for x in lib_hash(felts)], i
        assert (root.tolist(), n.value) == (logm.root(k), k)
        for r in led.receipts(range(k)):
            assert_receipt(r, model, logm, k)
        return leaves.tolist()
    finally:
        led.free()


def tampered(r, other, last):
    """(what, receipt) pairs that must not check: ballot_receipt_model.tampered's, with the ledger's
    fields for the ballot's, and the ledger's own.  `other`: another receipt of the same commitment;
    `last`: the receipt of its last entry."""
    sib = [list(d) for d in r.siblings]
    sib[-1][2] ^= 1
    a = r.amount
    assert a[0] != a[1]
    acc = list(r.account)
    acc[2] ^= 1
    return [("credited", r._replace(credited=not r.credited)),
            ("number", r._replace(number=r.number + 1)), ("sibling felt", r._replace(siblings=sib)),
            ("depth + 1", r._replace(depth=r.depth + 1, siblings=r.siblings + [[0, 0, 0, 0]])),
            ("depth - 1", r._replace(depth=r.depth - 1, siblings=r.siblings[:-1])),
            ("path bit", r._replace(path_bits=r.path_bits ^ 1)),
            ("top path bit", r._replace(path_bits=r.path_bits ^ (1 << (r.depth - 1)))),
            ("wrong n", last._replace(n=last.n + 1)), ("n at seq", last._replace(n=last.n - 1)),
            ("n = 0", r._replace(n=0)), ("n twice", r._replace(n=2 * r.n)),
            ("another entry's seq", r._replace(seq=other.seq)),
            ("non-canonical sibling", r._replace(siblings=[[P, 0, 0, 0]] + r.siblings[1:])),
            ("amount limb", r._replace(amount=[a[0], a[1], a[2] ^ 1, a[3]])),
            ("limbs swapped", r._replace(amount=[a[1], a[0], a[2], a[3]])),
            ("amount limb 2^32", r._replace(amount=[a[0], a[1], a[2], a[3] + (1 << 32)])),
            ("account felt", r._replace(account=acc)),
            ("non-canonical account", r._replace(account=[P] + list(r.account[1:]))),
            ("nullifier felt", r._replace(nullifier=[r.nullifier[0] ^ 1] + list(r.nullifier[1:])))]


def check_receipt_rules(ledger_factory):
    """a double spend's own receipt, every tampering, a receipt offered against a later commitment,
    and the refusals"""
    import pytest
    from qp_wormhole import QpError, WormholeLedger
    cap, roots, padding, items = make_stream("across_batches")
    model, logm = Model(roots, padding), LedgerLogModel()
    led = ledger_factory(roots, padding, cap)
    try:
        with pytest.raises(QpError, match="QP_ERR_STATE.*empty log"):
            led.commit_log()
        with pytest.raises(QpError, match="QP_ERR_STATE.*empty log"):
            led.receipts([0])
        with pytest.raises(QpError, match="QP_ERR_STATE.*empty log"):
            led.roots_at([1])
        half = items[:37]  # 32 credited transfers and five double spends
        cast_batch(led, half)
        for pi, v in half:
            model.cast_one(pi, v)
        logm.sync(model)
        n_a = len(model.log)
        pair = led.commit_log()
        assert pair == (logm.root(n_a), n_a) and led.commit_log() == pair  # nothing new: the same pair
        double = led.receipts([34])[0]  # a double spend's own entry
        assert not double.credited and double.seq == 34
        assert_receipt(double, model, logm, n_a)
        assert led.receipt_for(double.nullifier).seq == 2 and led.receipt_for([1, 2, 3, 4]) is None
        r, other, last = led.receipts([5, 20, n_a - 1])
        for x in (r, other, last):
            assert_receipt(x, model, logm, n_a)
        for what, bad in tampered(r, other, last):
            assert not WormholeLedger.check_receipt(bad), what
            assert not check_receipt(bad), what
        with pytest.raises(QpError, match="QP_ERR_ARG.*position 1"):
            led.receipts([0, n_a])
        with pytest.raises(QpError, match="QP_ERR_ARG.*position 2"):
            led.entries_at([0, 1, n_a])
        with pytest.raises(QpError, match="QP_ERR_ARG.*position 0"):
            led.roots_at([n_a + 1])
        assert led.commit_log() == pair
        # a later commitment: the old receipt holds under its own pair only
        cast_batch(led, items[37:])
        for pi, v in items[37:]:
            model.cast_one(pi, v)
        logm.sync(model)
        n_b = len(model.log)
        root_b, got_n = led.commit_log()
        assert (root_b, got_n) == (logm.root(n_b), n_b) and root_b != pair[0]
        assert WormholeLedger.check_receipt(r) and WormholeLedger.check_receipt(r, pair[0], n_a)
        for root, n in ((root_b, n_b), (root_b, n_a)):
            assert not WormholeLedger.check_receipt(r, root, n) and not check_receipt(r, root, n)
        again = led.receipts([5])[0]
        assert_receipt(again, model, logm, n_b)
        assert led.root_at(n_a) == pair[0]
        return [tuple(x) for x in (double, r, other, again)]
    finally:
        led.free()


def check_roots_at_every_m(ledger_factory, n=131):
    """roots_at of every m of an n-entry log equals the model's root at m"""
    led, model, logm = sized_ledger(ledger_factory, sized_items(n))
    try:
        got = led.roots_at(range(1, n + 1))
        assert got == [logm.root(m) for m in range(1, n + 1)]
        assert got[-1] == led.commit_log()[0] and led.root_at(1) == logm.leaves[0]
        assert led.roots_at([]) == [] and led.roots_at([n, 1, n]) == [got[-1], got[0], got[-1]]
        return got
    finally:
        led.free()


# ---- the audit's model.  A log is [(nullifier tuple, number, limbs tuple, account tuple, flags byte)];
# claimed totals are (credited, total int); claimed payouts [(account tuple, total int, first_seq)].

def log_of(entries):
    nul, num, amt, acc, credited = entries
    return [(tuple(int(x) for x in k), int(m), tuple(limbs_of(int(a))), tuple(int(x) for x in c), int(bool(f)))
            for k, m, a, c, f in zip(nul, num, amt, acc, credited)]


def arrays_of(log):
    """(nullifiers, numbers, amount limbs, accounts, flags) arrays of a model log, a form audit_ledger_log takes"""
    n = len(log)
    return (np.array([e[0] for e in log], dtype=np.uint64).reshape(n, 4), np.array([e[1] for e in log], dtype=np.uint64),
            np.array([e[2] for e in log], dtype=np.uint32).reshape(n, 4),
            np.array([e[3] for e in log], dtype=np.uint64).reshape(n, 4), np.array([e[4] for e in log], dtype=np.uint8))


def payouts_claim(payouts):
    """WormholeLedger.payouts()'s tuple form as the model's claim"""
    return [(tuple(int.from_bytes(a[i:i + 8], "little") for i in range(0, 32, 8)), int(t), int(s)) for a, t, s in payouts]


def amount_of(limbs):
    return sum(int(x) << (96 - 32 * i) for i, x in enumerate(limbs))


class Tree:
    """prefix roots of one canonical log: tree_from_leaves over the prefix, kept per m; logs above 300
    entries take most of them from LogModel's kept full nodes and hold the two equal at a few m"""

    def __init__(self, log):
        self.leaves = [hash_no_pad(list(k) + [m] + list(a) + list(c) + [f]) for k, m, a, c, f in log]
        self.kept, self.fast = {}, None
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


def audit(log, root=None, totals=None, payouts=None, commitments=()):
    """the model's verdict on `log` and the claims"""
    n = len(log)
    assert 1 <= n <= 1 << 31 and all(c[1] >= 1 for c in commitments)
    for seq, (nul, num, amt, acc, fl) in enumerate(log):
        if any(x >= P for x in nul + acc) or num >= P or fl > 1:
            return Report(NON_CANONICAL, seq, None, [0, 0, 0, 0], 0, 0, 0)
    order = next((seq for seq in range(1, n) if log[seq][1] <= log[seq - 1][1]), None)
    seen, rule, sums, first_seq, credited = {}, None, {}, {}, 0
    for seq, (nul, num, amt, acc, fl) in enumerate(log):
        first = seen.setdefault(nul, seq)
        if bool(fl & 1) != (first == seq) and rule is None:
            rule = (seq, first)
        if fl & 1:
            credited += 1
            first_seq.setdefault(acc, seq)
            sums[acc] = sums.get(acc, 0) + amount_of(amt)
    mine = [(acc, sums[acc], s) for acc, s in first_seq.items()]  # dicts keep the order of first insertion
    total = sum(sums.values())
    tree = Tree(log)
    rest = (tree.prefix_root(n), credited, total, len(mine))
    if order is not None:
        return Report(ORDER, order, None, *rest)
    if rule is not None:
        return Report(CREDIT_RULE, rule[0], rule[1], *rest)
    if totals is not None and tuple(totals) != (credited, total):
        return Report(TOTALS, None, None, *rest)
    if payouts is not None:
        claimed = [(tuple(a), int(t), int(s)) for a, t, s in payouts]
        k = min(len(claimed), len(mine))
        bad = next((i for i in range(k) if claimed[i] != mine[i]), None)
        if bad is None and len(claimed) != len(mine):
            bad = k
        if bad is not None:
            return Report(PAYOUTS, bad, None, *rest)
    if root is not None and list(root) != rest[0]:
        return Report(ROOT, None, None, *rest)
    for i, (r_i, n_i) in enumerate(commitments):
        if n_i > n or tree.prefix_root(n_i) != list(r_i):
            return Report(COMMITMENT, i, None, *rest)
    return Report(OK, None, None, *rest)


def same(rep, want):
    assert tuple(rep) == tuple(want), (tuple(rep), tuple(want))
    return tuple(rep)


# ---- the audit cases both paths run.  ctx: a Context or None, what audit_ledger_log runs on

def check_honest_stream(ctx, ledger_factory, name):
    """stream `name` through a real ledger in batches of 7, a commitment taken after every batch; the
    log audited with its own root, totals, payouts (both forms) and all the commitments"""
    from qp_wormhole import audit_ledger_log
    cap, roots, padding, items = make_stream(name)
    led = ledger_factory(roots, padding, cap)
    commitments = []
    try:
        for kind, arg in batches(items, 7):
            if kind == "reserve":
                led.reserve(arg)
                continue
            cast_batch(led, arg)
            if led.admitted:
                commitments.append(led.commit_log())
        if not led.admitted:
            return None
        root, n = led.commit_log()
        entries, payouts, raw = led.entries(), led.payouts(), led.payouts(raw=True)
        credited, admitted, total = led.recount()
    finally:
        led.free()
    assert n == admitted == len(entries[1]) and commitments[-1] == (root, n)
    commitments = commitments[::max(1, len(commitments) // 16)] + commitments[-1:]
    rep = audit_ledger_log(ctx, entries, root=root, totals=(credited, total), payouts=payouts, commitments=commitments)
    assert (rep.status, rep.witness, rep.first) == (OK, None, None)
    assert (rep.root, rep.credited, rep.total, rep.accounts) == (root, credited, total, len(payouts))
    assert audit_ledger_log(ctx, entries, root=root, totals=(credited, total), payouts=raw) == \
        rep._replace()  # the raw form of the payouts is the same claim
    return same(rep, audit(log_of(entries), root, (credited, total), payouts_claim(payouts), commitments))


# the tampering base: 700 entries, three blocks of 256 lanes, 9 accounts.  Double spends: 20 of 10 (one
# wave), 600 of 5 (different blocks), 300 of 299 (neighbours)
BASE_N, DOUBLES, BASE_MS = 700, {20: 10, 600: 5, 300: 299}, [100, 400, 650]


def base_log(ledger_factory):
    """(log, root, totals, payouts claim, commitments at BASE_MS) of the honest base, through a real ledger"""
    items = sized_items(BASE_N, seed=77, accounts=9)
    for d, first in DOUBLES.items():
        items[d] = (transfer(items[first][0][0:4], 1000 + d, items[d][0][12:16]), 0)
    led = ledger_factory([ROOT_A], None, BASE_N)
    try:
        cast_batch(led, items)
        root, n = led.commit_log()
        log, payouts = log_of(led.entries()), payouts_claim(led.payouts())
        credited, _, total = led.recount()
        commitments = list(zip(led.roots_at(BASE_MS), BASE_MS))
    finally:
        led.free()
    assert n == BASE_N and [s for s, e in enumerate(log) if not e[4]] == sorted(DOUBLES) and len(payouts) == 9
    return log, root, (credited, total), payouts, commitments


def _edit(log, **at):
    """a copy of log with entries replaced: _edit(log, s20=lambda k, m, a, c, f: (k, m, a, c, 1))"""
    out = list(log)
    for key, fn in at.items():
        s = int(key[1:])
        out[s] = fn(*out[s])
    return out


def _swap_numbers(log, a, b):
    out = list(log)
    out[a], out[b] = log[a][:1] + (log[b][1],) + log[a][2:], log[b][:1] + (log[a][1],) + log[b][2:]
    return out


def tamperings(log, root, totals, payouts, commitments):
    """[(what, log, claims, (status, witness, first))]: each tampering alone, the four payouts cases,
    two of one reason, two of two reasons.  claims = (root, totals, payouts, commitments)."""
    everything = (root, totals, payouts, commitments)
    set_credited = lambda k, m, a, c, f: (k, m, a, c, 1)  # noqa: E731
    felt_p = lambda k, m, a, c, f: (k[:2] + (P,) + k[3:], m, a, c, f)  # noqa: E731
    acc_p = lambda k, m, a, c, f: (k, m, a, c[:3] + (P,), f)  # noqa: E731
    limb = lambda k, m, a, c, f: (k, m, (a[0], a[1], a[2], a[3] ^ 1), c, f)  # noqa: E731
    assert log[7][4] and not log[300][4]
    rewritten = _edit(log, s300=limb)  # a double spend's amount: totals and payouts stay, every root from 301 on moves
    cheat_root = Tree(rewritten).prefix_root(len(log))
    off = list(payouts)
    off[3] = (off[3][0], off[3][1] + (1 << 32), off[3][2])  # limb sum 2 of account 3 off by one
    swapped = [payouts[0], payouts[2], payouts[1]] + payouts[3:]
    extra = payouts + [((1, 2, 3, 4), 5, 6)]
    seq_off = list(payouts)
    seq_off[8] = (seq_off[8][0], seq_off[8][1], seq_off[8][2] + 1)
    return [
        ("nullifier felt = p", _edit(log, s650=felt_p), everything, (NON_CANONICAL, 650, None)),
        ("account felt = p", _edit(log, s511=acc_p), everything, (NON_CANONICAL, 511, None)),
        ("number = p", _edit(log, s3=lambda k, m, a, c, f: (k, P, a, c, f)), everything, (NON_CANONICAL, 3, None)),
        ("flags = 2", _edit(log, s256=lambda k, m, a, c, f: (k, m, a, c, 2)), everything, (NON_CANONICAL, 256, None)),
        ("numbers swapped over a block edge", _swap_numbers(log, 255, 256), everything, (ORDER, 256, None)),
        ("numbers equal", _edit(log, s40=lambda k, m, a, c, f: (k, log[39][1], a, c, f)), everything, (ORDER, 40, None)),
        ("first transfer not credited", _edit(log, s10=lambda k, m, a, c, f: (k, m, a, c, 0)), everything,
         (CREDIT_RULE, 10, 10)),
        ("double spend credited, one wave", _edit(log, s20=set_credited), everything, (CREDIT_RULE, 20, 10)),
        ("double spend credited, other block", _edit(log, s600=set_credited), everything, (CREDIT_RULE, 600, 5)),
        ("amount changed, old totals", _edit(log, s7=limb), (None, totals, None, ()), (TOTALS, None, None)),
        ("credited count off", log, (root, (totals[0] + 1, totals[1]), payouts, commitments), (TOTALS, None, None)),
        ("amount changed, old payouts", _edit(log, s7=limb), (None, None, payouts, ()),
         (PAYOUTS, next(i for i, p in enumerate(payouts) if p[0] == log[7][3]), None)),
        ("one limb sum off by one", log, (root, totals, off, commitments), (PAYOUTS, 3, None)),
        ("two payouts swapped", log, (root, totals, swapped, commitments), (PAYOUTS, 1, None)),
        ("one payout dropped from the end", log, (root, totals, payouts[:-1], commitments), (PAYOUTS, 8, None)),
        ("one payout appended", log, (root, totals, extra, commitments), (PAYOUTS, 9, None)),
        ("no payouts claimed for a log with some", log, (root, totals, [], commitments), (PAYOUTS, 0, None)),
        ("first_seq off", log, (root, totals, seq_off, commitments), (PAYOUTS, 8, None)),
        ("amount changed, old root", _edit(log, s7=limb), (root, None, None, ()), (ROOT, None, None)),
        ("history rewritten", rewritten, (cheat_root, totals, payouts, commitments), (COMMITMENT, 1, None)),
        ("n_i > n", log, (root, totals, payouts, commitments[:1] + [(root, len(log) + 1)]), (COMMITMENT, 1, None)),
        ("two credited doubles in two blocks", _edit(log, s600=set_credited, s20=set_credited), everything,
         (CREDIT_RULE, 20, 10)),
        ("two non-canonical in two blocks", _edit(log, s650=felt_p, s3=acc_p), everything, (NON_CANONICAL, 3, None)),
        ("two swaps in two blocks", _swap_numbers(_swap_numbers(log, 610, 611), 30, 31), everything, (ORDER, 31, None)),
        ("order and credit rule", _edit(_swap_numbers(log, 500, 501), s20=set_credited), everything, (ORDER, 501, None)),
        ("non-canonical and order", _edit(_swap_numbers(log, 39, 40), s650=felt_p), everything,
         (NON_CANONICAL, 650, None)),
        ("credit rule, totals and root", _edit(log, s20=set_credited), everything, (CREDIT_RULE, 20, 10)),
        ("totals, payouts and root", _edit(log, s7=limb), everything, (TOTALS, None, None)),
        ("payouts and root", log, (cheat_root, totals, off, commitments), (PAYOUTS, 3, None)),
        ("root and commitment", rewritten, everything, (ROOT, None, None)),
    ]


def check_tamperings(ctx, ledger_factory):
    from qp_wormhole import audit_ledger_log
    log, root, totals, payouts, commitments = base_log(ledger_factory)
    honest = audit_ledger_log(ctx, arrays_of(log), root=root, totals=totals, payouts=payouts, commitments=commitments)
    out = [same(honest, audit(log, root, totals, payouts, commitments))]
    assert honest.status == OK
    for what, bad, (r, t, p, cs), want in tamperings(log, root, totals, payouts, commitments):
        before = [a.copy() for a in arrays_of(bad)]
        arrays = [a.copy() for a in before]
        rep = audit_ledger_log(ctx, tuple(arrays), root=r, totals=t, payouts=p, commitments=cs)
        assert (rep.status, rep.witness, rep.first) == want, what
        assert all((a == b).all() for a, b in zip(arrays, before)), what  # an audit never alters what it was given
        out.append(same(rep, audit(bad, r, t, p, cs)))
    return out


def check_counted_double_spend(ctx, ledger_factory):
    """a published log that credits a double spend: reason 3 with `first`, whatever else is claimed"""
    from qp_wormhole import audit_ledger_log
    cap, roots, padding, items = make_stream("one_nullifier")
    led = ledger_factory(roots, padding, cap)
    try:
        cast_batch(led, items)
        nul, num, amt, acc, credited = led.entries()
        root, payouts = led.commit_log()[0], led.payouts()
    finally:
        led.free()
    assert credited.tolist() == [True] + [False] * 63
    credited[41] = True
    rep = audit_ledger_log(ctx, (nul, num, amt, acc, credited), root=root, payouts=payouts)
    assert (rep.status, rep.witness, rep.first) == (CREDIT_RULE, 41, 0)
    return same(rep, audit(log_of((nul, num, amt, acc, credited)), root, None, payouts_claim(payouts)))


def check_big_totals(ctx, ledger_factory, n=4096):
    """n transfers of 2^128 - 1 to one account: the total is beyond 2^128 and audits exactly; one unit
    more or less in the claim is TOTALS, and PAYOUTS when only the payouts are claimed"""
    from qp_wormhole import audit_ledger_log
    rng = np.random.default_rng(4096)
    nuls = rng.integers(0, P, size=(n, 4), dtype=np.uint64).tolist()
    items = [(transfer(k, MAX_AMOUNT, [9, 8, 7, 6]), 0) for k in nuls]
    led = ledger_factory([ROOT_A], None, n)
    try:
        cast_batch(led, items)
        entries, payouts, recount = led.entries(), led.payouts(), led.recount()
    finally:
        led.free()
    total = n * MAX_AMOUNT
    assert total > 1 << 128 and recount == (n, n, total) and [p[1:] for p in payouts] == [(total, 0)]
    rep = audit_ledger_log(ctx, entries, totals=(n, total), payouts=payouts)
    assert (rep.status, rep.credited, rep.total, rep.accounts) == (OK, n, total, 1)
    out = [tuple(rep)]
    for delta in (1, -1, 1 << 96, -(1 << 128)):
        bad = audit_ledger_log(ctx, entries, totals=(n, total + delta), payouts=payouts)
        assert (bad.status, bad.witness, bad.total) == (TOTALS, None, total), delta
        bad = audit_ledger_log(ctx, entries, payouts=[(payouts[0][0], total + delta, 0)])
        assert (bad.status, bad.witness, bad.total) == (PAYOUTS, 0, total), delta
        out.append(tuple(bad))
    return out
