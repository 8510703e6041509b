"""The nullifier-set commitment as a plain-Python model: `sorted` on tuples, the
oracle's hash_no_pad and the accumulator-tree fold (registry_open_model.
tree_from_leaves).  Shared by the host-path and the device tests; nothing here
calls the code under test.

Definitions (include/qpgpu.h): the set = the log entries whose
member flag is set; the order = (nullifier as four unsigned words, seq); set
leaf at sorted position j = hash_no_pad([K_j[0..4], seq_j, 2]); the commitment
is (root, m), the zero root for m = 0; a proof for x is pos = the keys below x,
found, the leaf at pos - 1 (absence, pos > 0) and the leaf at pos (pos < m).
"""
import random

from oracle_lib import P, hash_no_pad
from registry_open_model import tree_from_leaves
from registry_oracle import oracle_path

PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4
ROOT_A = [11, 12, 13, P - 1]
OK, SHAPE, ROOT, NON_CANONICAL, NULL, ORDER = range(6)  # qp_nullifier_set_check's codes


class SetModel:
    def __init__(self, nullifiers, member):
        """nullifiers: n rows of 4 ints; member: n truthy flags"""
        recs = sorted((tuple(int(x) for x in nullifiers[s]), s) for s in range(len(member)) if member[s])
        self.keys = [list(k) for k, _ in recs]
        self.order = [s for _, s in recs]
        self.m = len(recs)
        dups = [self.order[j] for j in range(1, self.m) if self.keys[j] == self.keys[j - 1]]
        self.duplicate = min(dups) if dups else None
        self.levels = tree_from_leaves([hash_no_pad(k + [s, 2]) for k, s in zip(self.keys, self.order)]) if recs else None
        self.root = self.levels[-1][0] if recs else [0, 0, 0, 0]

    def leaf(self, j):
        """(key, seq, siblings, path_bits, depth) of sorted position j"""
        sibs, sides = oracle_path(self.levels, j)
        return (self.keys[j], self.order[j], [list(s) for s in sibs], sum(int(b) << i for i, b in enumerate(sides)),
                len(sibs))

    def proof(self, x):
        """(found, pos, lo, hi), lo / hi as `leaf` gives them or None"""
        x = [int(v) for v in x]
        pos = sum(1 for k in self.keys if k < x)
        found = pos < self.m and self.keys[pos] == x
        lo = self.leaf(pos - 1) if not found and pos > 0 else None
        hi = self.leaf(pos) if pos < self.m else None
        return found, pos, lo, hi


def as_tuple(p):
    """a NullifierProof as the model's (found, pos, lo, hi)"""
    return p.found, p.pos, None if p.lo is None else tuple(p.lo), None if p.hi is None else tuple(p.hi)


def model_tuple(t):
    found, pos, lo, hi = t
    return found, pos, None if lo is None else tuple(lo), None if hi is None else tuple(hi)


def between(a, b):
    """a canonical key strictly between keys a < b: a's successor in felt 3, if it is one"""
    k = list(a[:3]) + [a[3] + 1]
    return k if k[3] < P and k < list(b) else None


def queries(model, rng, extra=8):
    """keys below all, above all, between each adjacent pair (where one exists), equal to each member,
    and a few random ones"""
    q = [[0, 0, 0, 0], [P - 1] * 4] + [list(k) for k in model.keys]
    for a, b in zip(model.keys, model.keys[1:]):
        k = between(a, b) if a != b else None
        if k is not None:
            q.append(k)
    q += [[rng.randrange(P) for _ in range(4)] for _ in range(extra)]
    return q


def random_keys(rng, n):
    return [[rng.randrange(P) for _ in range(4)] for _ in range(n)]


def pattern_keys(name, n, slots=None):
    """n distinct canonical keys of the named pattern (the shapes where a sort or a merge breaks)"""
    rng = random.Random("nset " + name)
    if name == "random":
        return random_keys(rng, n)
    if name == "sorted":
        return sorted(random_keys(rng, n))
    if name == "reverse":
        return sorted(random_keys(rng, n), reverse=True)
    if name == "felt3_only":  # equal in felts 0..2
        pre = [rng.randrange(P) for _ in range(3)]
        return [pre + [v] for v in rng.sample(range(1 << 40), n)]
    if name == "high32_only":  # felt 0 equal in its low 32 bits, differing in the high 32
        low = rng.randrange(1 << 32)
        rest = [rng.randrange(P) for _ in range(3)]
        return [[(h << 32) | low] + rest for h in rng.sample(range((1 << 32) - 1), n)]
    if name == "low32_only":  # the converse; a high half with bit 31 set, so a signed compare differs
        high = 0x80000001 << 32
        rest = [rng.randrange(P) for _ in range(3)]
        return [[high | v] + rest for v in rng.sample(range(1 << 32), n)]
    if name == "edges":  # felts at 0 and p - 1, and values either side of 2^63 and 2^32
        vals = [0, P - 1, 1, P - 2, 1 << 63, (1 << 63) - 1, 1 << 32, (1 << 32) - 1]
        seen, out = set(), []
        while len(out) < n:
            k = tuple(rng.choice(vals) if rng.random() < 0.8 else rng.randrange(P) for _ in range(4))
            if k not in seen:
                seen.add(k)
                out.append(list(k))
        return out
    if name == "one_home":  # every key's home slot in the handle's table is the same
        return [[(v * slots) | 5, rng.randrange(P), rng.randrange(P), rng.randrange(P)]
                for v in rng.sample(range(1, 1 << 30), n)]
    raise ValueError(name)


PATTERNS = ["random", "sorted", "reverse", "felt3_only", "high32_only", "low32_only", "edges", "one_home"]


def ballot(nullifier, vote=1):
    return PROPOSAL + ROOT_A + [vote] + [int(x) for x in nullifier]


def transfer(nullifier, amount=1, account=(1, 2, 3, 4)):
    return [int(x) for x in nullifier] + ROOT_A + [0, 0, 0, amount] + list(account)


def make_handle(kind, ctx, capacity):
    import qp_wormhole
    if kind == "box":
        return qp_wormhole.BallotBox(ctx, PROPOSAL, [ROOT_A], capacity=capacity)
    return qp_wormhole.WormholeLedger(ctx, [ROOT_A], capacity=capacity)


def cast_keys(kind, h, keys):
    """admits one entry per key, in order; returns the statuses"""
    import numpy as np
    make = ballot if kind == "box" else transfer
    pis = np.array([make(k) for k in keys], dtype=np.uint64)
    return [int(s) for s in h.cast_public(pis, raw=True)["status"]]


def handle_log(kind, h):
    """(nullifiers rows, member flags) of a handle's log"""
    e = h.entries()
    member = e[2] if kind == "box" else e[4]
    return [[int(x) for x in r] for r in e[0]], [bool(x) for x in member]


def shape(j, m):
    """(depth, path_bits) of leaf j in a tree of m leaves: the (j, m) shape rule"""
    d = bits = l = 0
    n = m
    while n > 1:
        if ((j >> l) ^ 1) < n:
            bits |= ((j >> l) & 1) << d
            d += 1
        n = (n + 1) // 2
        l += 1
    return d, bits


ZERO_LEAF = ([0, 0, 0, 0], 0, [], 0, 0)


def model_check(x, found, pos, lo, hi, root, m):
    """the checker's rules, independently: the first reason in the order non-canonical, shape, order,
    root.  lo / hi: (key, seq, siblings, path_bits, depth) or None (an all-zero slot); a slot's
    siblings list is as long as its depth."""
    lo, hi = lo or ZERO_LEAF, hi or ZERO_LEAF
    felts = list(root) + list(x)
    for s in (lo, hi):
        felts += list(s[0]) + [s[1]] + [f for d in s[2] for f in d]
    if any(f >= P for f in felts):
        return NON_CANONICAL
    if m > 1 << 31 or pos > m or found > 1 or (found and pos == m):
        return SHAPE
    has = (not found and pos > 0, pos < m)
    at = (pos - 1, pos)
    for s, h, j in zip((lo, hi), has, at):
        if not h:
            if tuple(s) != tuple(ZERO_LEAF) and (list(s[0]), s[1], list(s[2]), s[3], s[4]) != list(ZERO_LEAF):
                return SHAPE
        elif (s[4], s[3]) != shape(j, m):
            return SHAPE
    if found:
        if list(hi[0]) != list(x):
            return ORDER
    else:
        if has[0] and not list(lo[0]) < list(x):
            return ORDER
        if has[1] and not list(x) < list(hi[0]):
            return ORDER
    if m == 0:
        return ROOT if any(root) else OK
    for s, h in zip((lo, hi), has):
        if not h:
            continue
        cur = hash_no_pad(list(s[0]) + [s[1], 2])
        for i, sib in enumerate(s[2]):
            cur = hash_no_pad(list(sib) + cur) if s[3] >> i & 1 else hash_no_pad(cur + list(sib))
        if cur != list(root):
            return ROOT
    return OK
