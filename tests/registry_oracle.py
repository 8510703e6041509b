"""The reference's eligibility-tree builder (voting/src/lib.rs:285-316) restated
over the oracle's hash_no_pad (test infrastructure): independent of the
product's registry code, host or device."""
import numpy as np

from edge_values import CANON_EDGES
from oracle_lib import P, hash_no_pad


def oracle_tree(keys):
    """levels[l] = list of digests; level 0 the leaves, the last level the root."""
    cur = [hash_no_pad(k) for k in keys]
    levels = [cur]
    while len(cur) > 1:
        nxt = []
        for i in range(0, len(cur), 2):
            nxt.append(hash_no_pad(cur[i] + cur[i + 1]) if i + 1 < len(cur) else cur[i])
        levels.append(nxt)
        cur = nxt
    return levels


def oracle_path(levels, i):
    """(siblings, path_indices) of voter i: the levels where its node was hashed."""
    sibs, path = [], []
    for lv in levels[:-1]:
        if i ^ 1 < len(lv):
            sibs.append(lv[i ^ 1])
            path.append(bool(i & 1))
        i >>= 1
    return sibs, path


def root_from_path(key, sibs, path):
    """the circuit's walk (voting/src/lib.rs:123-180) over a compacted path"""
    cur = hash_no_pad(key)
    for s, right in zip(sibs, path):
        cur = hash_no_pad(list(s) + cur if right else cur + list(s))
    return cur


def make_keys(n, seed=0):
    """n keys [n][4]: random canonical felts, and edge-value keys (0, 1, p - 1,
    2^32 - 1 patterns, ...) at the first, the last and every 7th voter."""
    rng = np.random.default_rng(0xE1EC7 + seed)
    k = rng.integers(0, P, size=(n, 4), dtype=np.uint64)
    ne = len(CANON_EDGES)
    for j, i in enumerate(sorted(set([0, n - 1] + list(range(0, n, 7))))):
        k[i] = [CANON_EDGES[(j + c) % ne] for c in range(4)] if j % 3 else [CANON_EDGES[j % ne]] * 4
    return k


