"""The payout claims commitment as a plain-Python model: a dict of exact integer
totals over the credited entries of a range, `sorted` on account tuples, five
limbs by divmod, the oracle's hash_no_pad, the accumulator-tree fold
(registry_open_model.tree_from_leaves) and the checker's rules.  Shared by the
host-path and the device tests; nothing here calls the code under test.

Definitions (include/qpgpu.h): for a log range [m0, m1) one row per
account with a credited entry in it: its exact total over those entries and
first_seq, the lowest such seq; rows sorted by account (four unsigned words,
felt 0 first); claim leaf at sorted position j = hash_no_pad([account[0..4],
t[0..5], first_seq, 3]) with t the total's five 32-bit limbs, most significant
first; the commitment is (root, A, total), the zero root for A = 0; a claim for
x is pos = the rows below x, found, the leaf at pos - 1 (absence, pos > 0) and
the leaf at pos (pos < A).
"""
import random

import numpy as np

from nullifier_set_model import ROOT_A, shape
from oracle_lib import P, hash_no_pad
from registry_open_model import tree_from_leaves
from registry_oracle import oracle_path

OK, SHAPE, ROOT, NON_CANONICAL, NULL, ORDER = range(6)  # qp_ledger_claim_check's codes
ROOT_B = [21, 22, 23, 24]  # a storage root no ledger here accepts
LEAF_TAG = 3


def limbs5(total):
    out = []
    for _ in range(5):
        total, r = divmod(total, 1 << 32)
        out.append(r)
    assert total == 0
    return out[::-1]


class ClaimsModel:
    def __init__(self, accounts, amounts, credited, m0=0, m1=None):
        """the log: accounts n rows of 4 ints, amounts n exact ints, credited n truthy flags"""
        m1 = len(credited) if m1 is None else m1
        owed = {}
        for seq in range(m0, m1):
            if credited[seq]:
                row = owed.setdefault(tuple(int(x) for x in accounts[seq]), [0, seq])
                row[0] += int(amounts[seq])
        rows = sorted(owed.items())
        self.accounts = [list(a) for a, _ in rows]
        self.totals = [r[0] for _, r in rows]
        self.order = [r[1] for _, r in rows]
        self.count = len(rows)
        self.total = sum(self.totals)
        leaves = [hash_no_pad(a + limbs5(t) + [s, LEAF_TAG]) for a, t, s in zip(self.accounts, self.totals, self.order)]
        self.levels = tree_from_leaves(leaves) if rows else None
        self.root = self.levels[-1][0] if rows else [0, 0, 0, 0]

    def leaf(self, j):
        """(account, total, first_seq, siblings, path_bits, depth) of sorted position j"""
        sibs, sides = oracle_path(self.levels, j)
        return (self.accounts[j], self.totals[j], self.order[j], [list(s) for s in sibs],
                sum(int(b) << i for i, b in enumerate(sides)), len(sibs))

    def claim(self, x):
        """(found, pos, lo, hi), lo / hi as `leaf` gives them or None"""
        x = [int(v) for v in x]
        pos = sum(1 for a in self.accounts if a < x)
        found = pos < self.count and self.accounts[pos] == x
        lo = self.leaf(pos - 1) if not found and pos > 0 else None
        hi = self.leaf(pos) if pos < self.count else None
        return found, pos, lo, hi


def as_tuple(p):
    """a PayoutClaim as the model's (found, pos, lo, hi)"""
    return p.found, p.pos, None if p.lo is None else tuple(p.lo), None if p.hi is None else tuple(p.hi)


def model_tuple(t):
    found, pos, lo, hi = t
    return found, pos, None if lo is None else tuple(lo), None if hi is None else tuple(hi)


ZERO_LEAF = ([0, 0, 0, 0], 0, 0, [], 0, 0)


def model_check(x, found, pos, lo, hi, root, count):
    """the checker's rules, independently: the first reason in the order non-canonical, shape, order,
    root.  lo / hi: (account, total, first_seq, siblings, path_bits, depth) or None (an all-zero
    slot); a slot's siblings list is as long as its depth."""
    lo, hi = lo or ZERO_LEAF, hi or ZERO_LEAF
    felts = list(root) + list(x)
    for s in (lo, hi):
        felts += list(s[0]) + [s[2]] + [f for d in s[3] for f in d]
    if any(f >= P for f in felts):
        return NON_CANONICAL
    if count > 1 << 31 or pos > count or found > 1 or (found and pos == count):
        return SHAPE
    has = (not found and pos > 0, pos < count)
    at = (pos - 1, pos)
    for s, h, j in zip((lo, hi), has, at):
        if not h:
            if (list(s[0]), s[1], s[2], list(s[3]), s[4], s[5]) != ZERO_LEAF:
                return SHAPE
        elif (s[5], s[4]) != shape(j, count):
            return SHAPE
    if found:
        if list(hi[0]) != list(x):
            return ORDER
    else:
        if has[0] and not list(lo[0]) < list(x):
            return ORDER
        if has[1] and not list(x) < list(hi[0]):
            return ORDER
    if count == 0:
        return ROOT if any(root) else OK
    for s, h in zip((lo, hi), has):
        if not h:
            continue
        cur = hash_no_pad(list(s[0]) + limbs5(s[1]) + [s[2], LEAF_TAG])
        for i, sib in enumerate(s[3]):
            cur = hash_no_pad(list(sib) + cur) if s[4] >> i & 1 else hash_no_pad(cur + list(sib))
        if cur != list(root):
            return ROOT
    return OK


def between(a, b):
    """a canonical account strictly between accounts a < b: a's successor in felt 3, if it is one"""
    k = list(a[:3]) + [a[3] + 1]
    return k if k[3] < P and k < list(b) else None


def queries(model, rng, extra=4):
    """accounts below all, above all, between each adjacent pair (where one exists), each member, a few random"""
    q = [[0, 0, 0, 0], [P - 1] * 4] + [list(a) for a in model.accounts]
    for a, b in zip(model.accounts, model.accounts[1:]):
        k = between(a, b)
        if k is not None:
            q.append(k)
    q += [[rng.randrange(P) for _ in range(4)] for _ in range(extra)]
    return q


def random_accounts(rng, n):
    return [[rng.randrange(P) for _ in range(4)] for _ in range(n)]


def pattern_accounts(name, n):
    """n distinct canonical accounts of the named pattern"""
    rng = random.Random("claims " + name)
    if name == "random":
        return random_accounts(rng, n)
    if name == "felt3_only":  # equal in felts 0..2
        pre = [rng.randrange(P) for _ in range(3)]
        return [pre + [v] for v in rng.sample(range(1 << 40), n)]
    if name == "high32_only":  # felt 0 equal in its low 32 bits, differing in the high 32
        low = rng.randrange(1 << 32)
        rest = [rng.randrange(P) for _ in range(3)]
        return [[(h << 32) | low] + rest for h in rng.sample(range((1 << 32) - 1), n)]
    if name == "edges":  # felts 0 and p - 1
        seen, out = set(), []
        while len(out) < n:
            k = tuple(rng.choice((0, P - 1)) if rng.random() < 0.75 else rng.randrange(P) for _ in range(4))
            if k not in seen:
                seen.add(k)
                out.append(list(k))
        return out
    raise ValueError(name)


PATTERNS = ["felt3_only", "high32_only", "edges"]
MAX_AMOUNT = (1 << 128) - 1  # every limb 0xFFFFFFFF


def amount_limbs(a):
    return [(a >> (96 - 32 * i)) & 0xFFFFFFFF for i in range(4)]


class Stream:
    """A transfer stream in the making: credited transfers (fresh nullifiers), double spends of an
    earlier nullifier (admitted to the log, not credited) and transfers under an unknown root (not
    admitted at all).  `pis()` is what cast_public takes."""

    def __init__(self, tag):
        self.rng = random.Random("claims stream " + str(tag))
        self.rows = []
        self.nullifiers = []

    def _nullifier(self):
        return [self.rng.randrange(P) for _ in range(4)]

    def credit(self, account, amount):
        n = self._nullifier()
        self.nullifiers.append(n)
        self.rows.append(n + ROOT_A + amount_limbs(amount) + [int(x) for x in account])

    def double(self, account, amount=7):
        self.rows.append(self.rng.choice(self.nullifiers) + ROOT_A + amount_limbs(amount) + [int(x) for x in account])

    def unknown_root(self, account, amount=9):
        self.rows.append(self._nullifier() + ROOT_B + amount_limbs(amount) + [int(x) for x in account])

    def pis(self):
        return np.array(self.rows, dtype=np.uint64).reshape(len(self.rows), 16)


def new_ledger(ctx, capacity):
    import qp_wormhole
    return qp_wormhole.WormholeLedger(ctx, [ROOT_A], capacity=max(capacity, 1))


def cast(led, stream):
    pis = stream.pis() if isinstance(stream, Stream) else stream
    if len(pis):
        led.cast_public(pis, raw=True)


def model_of(led, m0=0, m1=None):
    """the model over a ledger's own log"""
    _, _, amounts, accounts, credited = led.entries()
    return ClaimsModel([[int(x) for x in a] for a in accounts], amounts, [bool(c) for c in credited], m0, m1)


def mixed_stream(tag, accounts, per_account=(1, 2, 3), amounts=None):
    """one to three credited entries per account in a shuffled order, a double spend after every
    fourth credit and a transfer under an unknown root after every fifth"""
    s = Stream(tag)
    todo = [a for i, a in enumerate(accounts) for _ in range(per_account[i % len(per_account)])]
    s.rng.shuffle(todo)
    for i, a in enumerate(todo):
        s.credit(a, s.rng.randrange(1 << 128) if amounts is None else amounts(a))
        if i % 4 == 3:
            s.double(s.rng.choice(accounts))
        if i % 5 == 4:
            s.unknown_root(a)
    return s
