"""The reference's eligibility-tree level loop (voting/src/lib.rs:292-316) over
the oracle's hash_no_pad, started from leaf digests instead of keys: the model
of a commitment registry after any sequence of appends and replaces is this
loop over the current list of commitments.  Shared by the host-fallback and
the device tests of the open (append / replace) registry, with the growth and
replace cases both run."""
import numpy as np

from oracle_lib import hash_no_pad
from registry_oracle import make_keys, oracle_path

# growth sequences: the sizes after the build and after each append, and the
# capacity the registry starts with (None: the default)
GROWTH = {
    "0-5": ([0, 1, 2, 3, 4, 5, 6], 8),            # empty start, first level, promoted node hashed at last, new level
    "fold-edge": ([63, 64, 65, 127, 130], None),  # REG_FOLD_MAX on the leaf level and the one above
    "1-200": ([1, 200], 1),                       # one call over many levels; the Python append reserves first
    "4095-4097": ([2**12 - 1, 2**12 + 1], None),
}
REPLACE_SIZES = [1, 2, 5, 65, 131]


def tree_from_leaves(leaves):
    """levels[l] = list of digests; level 0 the given leaves, the last level the root."""
    cur = [[int(x) for x in d] for d in leaves]
    levels = [cur]
    while len(cur) > 1:
        nxt = []
        for i in range(0, len(cur), 2):
            nxt.append(hash_no_pad(cur[i] + cur[i + 1]) if i + 1 < len(cur) else cur[i])
        levels.append(nxt)
        cur = nxt
    return levels


def make_commitments(n, seed=0):
    """n leaf digests [n][4]: canonical felts, edge values among them (not hashes
    of known keys: the tree does not care)"""
    return make_keys(n, 1000 + seed) if n else np.zeros((0, 4), np.uint64)


def check_tree(reg, leaves, voters, other=None):
    """reg's size, root, every level and the paths of `voters` equal the model's
    over `leaves` (and `other`'s, a second registry of the same list)"""
    n = len(leaves)
    lv = tree_from_leaves(leaves)
    assert (reg.size, reg.num_levels, reg.max_depth) == (n, len(lv), len(lv) - 1)
    assert reg.root == lv[-1][0]
    for l, want in enumerate(lv):
        got = reg.level(l)
        assert got.shape == (len(want), 4), l
        assert got.tolist() == want, (n, l)
        if other is not None:
            assert other.level(l).tolist() == want, (n, l)
    voters = sorted({v for v in voters if 0 <= v < n})
    sibs, path, depth = reg.paths(voters)
    for b, i in enumerate(voters):
        osib, opath = oracle_path(lv, i)
        assert (sibs[b], path[b], depth[b]) == (osib, opath, len(osib)), (n, i)
    if other is not None:
        assert other.root == reg.root
        for a, b in zip(reg.paths_raw(voters), other.paths_raw(voters)):
            assert np.array_equal(a, b)
    return lv


def run_growth(ctx, name, other_ctx="none"):
    """the growth sequence `name` on a registry of ctx (None: the host
    fallback), checked after every step; other_ctx != "none": a second
    registry of that context taken through the same steps and compared"""
    from qp_wormhole import VoterRegistry
    sizes, cap = GROWTH[name]
    leaves = make_commitments(sizes[-1], len(name))
    regs = [VoterRegistry.from_commitments(c, leaves[:sizes[0]], capacity=cap)
            for c in ([ctx] if other_ctx == "none" else [ctx, other_ctx])]
    try:
        reg, other = regs[0], (regs[1] if len(regs) > 1 else None)
        assert reg.epoch == 0 and not reg.has_keys and reg.capacity == (cap or max(2 * sizes[0], 1024))
        if sizes[0]:
            check_tree(reg, leaves[:sizes[0]], [0, sizes[0] - 1], other)
        else:
            assert (reg.size, reg.num_levels, reg.root) == (0, 0, None)
        for step, (n_old, n) in enumerate(zip(sizes, sizes[1:])):
            for r in regs:
                assert r.append(leaves[n_old:n]) == n_old
            check_tree(reg, leaves[:n], [0, n_old - 1, n_old, n - 1], other)
            assert reg.capacity >= n and reg.epoch >= step + 1
    finally:
        for r in regs:
            r.free()


def replace_cases(n):
    """index lists for a registry of n voters: voter 0, the last (a promoted
    lone node at one or more levels for odd n), both children of one parent,
    every voter"""
    cases = [[0], [n - 1]]
    if n >= 2:
        cases.append([1, 0])
        cases.append([n - 1, (n - 1) ^ 1] if (n - 1) ^ 1 < n else [n - 2, n - 3])
    cases.append(list(range(n - 1, -1, -1)))
    return cases


def run_replace(ctx, n, other_ctx="none"):
    from qp_wormhole import VoterRegistry
    leaves = make_commitments(n, n).tolist()
    fresh = make_commitments(4 * n + 4, 7 * n).tolist()
    regs = [VoterRegistry.from_commitments(c, leaves) for c in ([ctx] if other_ctx == "none" else [ctx, other_ctx])]
    try:
        reg, other = regs[0], (regs[1] if len(regs) > 1 else None)
        for step, idx in enumerate(replace_cases(n)):
            new = [fresh.pop() for _ in idx]
            for i, d in zip(idx, new):
                leaves[i] = d
            for r in regs:
                r.replace(idx, new)
            check_tree(reg, leaves, [0, n - 1] + idx[:4], other)
            assert reg.epoch == step + 1 and reg.size == n
        again = VoterRegistry.from_commitments(ctx, leaves)  # a fresh build of the edited list
        try:
            assert again.root == reg.root
            for l in range(reg.num_levels):
                assert np.array_equal(again.level(l), reg.level(l)), l
        finally:
            again.free()
    finally:
        for r in regs:
            r.free()
