"""VoterRegistry: the electorate's Merkle tree of one proposal and the Merkle
paths the voting circuit takes (VotePrivateInputs.merkle_siblings,
path_indices, actual_merkle_depth; merkle_root public), by voter index.

The tree is the one the reference's test builds with a host loop
(voting/src/lib.rs:285-316) and its circuit walks (:123-180):

  leaf = hash_no_pad(4-felt private key)
  node = hash_no_pad(left || right)
  the last node of an odd-length level moves to the next level unchanged

so N need not be a power of two, and a voter's path is the compacted list of
the siblings of the levels where its node was actually hashed.

With a Context (or a device number) the tree is built and kept on the device
(qp_registry_*, csrc/registry.hip) and `prove` fills the prover's inputs from
the device paths (qp_prover_prove_voters).  With None the same tree is built on
the host through qp_hash_no_pad, one call per node: for small electorates and
as the device path's cross-check.

Two kinds.  VoterRegistry(ctx, keys) is the custodial one: it hashes the keys
itself and keeps them for `inputs` / `prove`.  VoterRegistry.from_commitments
is the election operator's: it holds only the leaves voters sent in
(`commitment(key)`), reserves `capacity` leaves so the tree grows in place,
and is updated by `append` / `replace` (qp_registry_append / _replace: only
the changed nodes are recomputed).  The operator publishes `root` and serves
`paths`; a voter builds their inputs with `inputs_for(key, index, ...)`.  Every
completed append, replace or reserve raises `epoch`; a path is valid only
under the root of the epoch it was taken in.
"""
import ctypes

import numpy as np

from ._native import Context, hash_no_pad, lib
from .circuits import U64_4, VoteCircuitData, VotePrivateInputs, VotePublicInputs

P = 0xFFFFFFFF00000001
PATH_SLOTS = 32          # MAX_MERKLE_DEPTH (voting/src/lib.rs:20)
MAX_DEPTH = 31           # depth 32 does not fit the circuit's 5-bit depth split
MAX_VOTERS = 1 << MAX_DEPTH
MIN_CAPACITY = 1024      # from_commitments(capacity=None) reserves max(2 n, this)
HOST_MAX_VOTERS = 1 << 17  # the host fallback hashes one node per Python call


class _Ballot(ctypes.Structure):
    """qp_vote_ballot"""
    _fields_ = [("proposal_id", U64_4), ("vote", ctypes.c_uint8), ("zk_randomness", ctypes.POINTER(ctypes.c_uint64))]


def _digest(v, what):
    d = [int(x) for x in v]
    if len(d) != 4 or any(not 0 <= x < P for x in d):
        raise ValueError(f"{what} must be 4 canonical field elements")
    return d


class VoterRegistry:
    def __init__(self, ctx_or_device, keys):
        """keys: [N][4] canonical felts, one private key per voter, in voter-index
        order.  ctx_or_device: a Context, a device number (an own Context), or
        None for the host fallback."""
        try:
            k = np.ascontiguousarray(keys, dtype=np.uint64)
        except OverflowError:
            raise ValueError("a key felt does not fit 64 bits, so it is not a field element") from None
        if k.size == 0:
            raise ValueError("a voter registry needs at least one voter (no keys given)")
        if k.ndim != 2 or k.shape[1] != 4:
            raise ValueError("keys must be [N][4] field elements")
        bad = np.argwhere(k >= np.uint64(P))
        if len(bad):
            raise ValueError(f"key {int(bad[0][0])} felt {int(bad[0][1])} is not a canonical field element (>= p)")
        n = k.shape[0]
        if (n - 1).bit_length() > MAX_DEPTH:
            raise ValueError(f"{n} voters need a Merkle path deeper than {MAX_DEPTH}, the most the voting circuit holds")
        self.keys = k
        self._set_size(n)
        self._capacity, self._epoch = n, 0
        self.h = self._levels = self._own_ctx = None
        if ctx_or_device is None:
            self.ctx = None
            self._build_host()
        else:
            self._open(ctx_or_device)
            h = ctypes.c_void_p()
            self.ctx.check(lib().qp_registry_new(self.ctx.h, k, n, ctypes.byref(h)), "qp_registry_new")
            self.h = h
            root = np.zeros(4, np.uint64)
            self.ctx.check(lib().qp_registry_root(self.h, root), "qp_registry_root")
            self.root = [int(x) for x in root]

    # ---- host fallback: the reference's loop (voting/src/lib.rs:292-316)
    def _build_host(self):
        if self.size > HOST_MAX_VOTERS:
            raise ValueError(f"the host fallback builds at most {HOST_MAX_VOTERS} voters; give a device for {self.size}")
        cur = [hash_no_pad(key) for key in self.keys]
        levels = [cur]
        while len(cur) > 1:
            nxt = [hash_no_pad(cur[i] + cur[i + 1]) if i + 1 < len(cur) else cur[i] for i in range(0, len(cur), 2)]
            levels.append(nxt)
            cur = nxt
        self._levels = [np.array(lv, dtype=np.uint64).reshape(-1, 4) for lv in levels]
        self.root = [int(x) for x in self._levels[-1][0]]

    def _set_size(self, n):
        self.size = n
        self.max_depth = (n - 1).bit_length() if n else 0
        self.num_levels = self.max_depth + 1 if n else 0

    def _open(self, ctx_or_device):
        if isinstance(ctx_or_device, Context):
            self.ctx = ctx_or_device
        else:
            self.ctx = self._own_ctx = Context(int(ctx_or_device))

    # ---- a registry from commitments (qp_registry_new_commitments, _append, _replace, _reserve)
    @staticmethod
    def commitment(key):
        """hash_no_pad(key): the leaf a voter sends in when registering."""
        return hash_no_pad(_digest(key, "a private key"))

    @staticmethod
    def _leaves(leaves, first=None, idx=None):
        """[k][4] canonical commitments; a bad felt names voter first + i (or idx[i])"""
        try:
            a = np.ascontiguousarray(leaves, dtype=np.uint64)
        except OverflowError:
            raise ValueError("a commitment felt does not fit 64 bits, so it is not a field element") from None
        if a.size == 0:
            return np.zeros((0, 4), np.uint64)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("commitments must be [k][4] field elements")
        bad = np.argwhere(a >= np.uint64(P))
        if len(bad):
            i, f = int(bad[0][0]), int(bad[0][1])
            who = int(idx[i]) if idx is not None else (first or 0) + i
            raise ValueError(f"commitment {who} (position {i} of the batch) felt {f} is not a canonical field "
                             "element (>= p)")
        return a

    @staticmethod
    def _check_capacity(n, capacity):
        if not max(n, 1) <= capacity <= MAX_VOTERS:
            raise ValueError(f"capacity {capacity} for {n} voters: it must hold them (and at least one) and be at "
                             f"most 2^{MAX_DEPTH}, the most voters a path of depth {MAX_DEPTH} reaches")

    @classmethod
    def from_commitments(cls, ctx_or_device, leaves, capacity=None):
        """The operator's registry: leaves [n][4], each a voter's commitment(key), in
        voter-index order; n may be 0.  capacity (default max(2 n, 1024)) leaves are
        reserved, so `append` grows the tree in place.  No keys are held."""
        a = cls._leaves(leaves, first=0)
        n = a.shape[0]
        capacity = min(max(2 * n, MIN_CAPACITY), max(n, MAX_VOTERS)) if capacity is None else int(capacity)
        cls._check_capacity(n, capacity)
        self = cls.__new__(cls)
        self.keys = None
        self._set_size(0)
        self._capacity, self._epoch = capacity, 0
        self.h = self._levels = self._own_ctx = None
        self.root = None
        if ctx_or_device is None:
            self.ctx = None
            self._levels = []
            if n:
                self._host_append(a)
            return self
        self._open(ctx_or_device)
        h = ctypes.c_void_p()
        self.ctx.check(lib().qp_registry_new_commitments(self.ctx.h, a.ctypes.data, n, capacity, ctypes.byref(h)),
                       "qp_registry_new_commitments")
        self.h = h
        self._refresh()
        return self

    def _refresh(self):
        """size and root of a device registry after an update"""
        n = ctypes.c_uint64()
        self.ctx.check(lib().qp_registry_size(self.h, ctypes.byref(n), None), "qp_registry_size")
        self._set_size(n.value)
        if n.value:
            root = np.zeros(4, np.uint64)
            self.ctx.check(lib().qp_registry_root(self.h, root), "qp_registry_root")
            self.root = [int(x) for x in root]

    @property
    def has_keys(self):
        return self.keys is not None

    def _state(self):
        if self.h is None:
            return self._capacity, self._epoch
        cap, ep = ctypes.c_uint64(), ctypes.c_uint64()
        self.ctx.check(lib().qp_registry_state(self.h, ctypes.byref(cap), ctypes.byref(ep)), "qp_registry_state")
        return cap.value, ep.value

    @property
    def capacity(self):
        return self._state()[0]

    @property
    def epoch(self):
        """completed append / replace / reserve calls; paths belong to one epoch's root"""
        return self._state()[1]

    def _no_keys(self, what):
        if self.keys is not None:
            raise ValueError(f"{what}: this registry was built from private keys and keeps a copy of them, which an "
                             "update would leave stale; build it with from_commitments")

    def _host_node(self, l, j):
        src = self._levels[l - 1]
        return hash_no_pad(src[2 * j] + src[2 * j + 1]) if 2 * j + 1 < len(src) else src[2 * j]

    def _host_append(self, a):
        """the device's dirty-range rule on the host: level l changes in [n_old >> l, ceil(n / 2^l))"""
        n_old, lv = self.size, self._levels
        if self.size + len(a) > HOST_MAX_VOTERS:
            raise ValueError(f"the host fallback holds at most {HOST_MAX_VOTERS} voters; give a device")
        if not lv:
            lv.append([])
        lv[0].extend([int(x) for x in row] for row in a)
        l = 1
        while len(lv[l - 1]) > 1:
            if l == len(lv):
                lv.append([])
            first, end = n_old >> l, (len(lv[l - 1]) + 1) // 2
            del lv[l][first:]
            lv[l].extend(self._host_node(l, j) for j in range(first, end))
            l += 1
        self._set_size(len(lv[0]))
        self.root = list(lv[-1][0])

    def append(self, leaves, reserve=True):
        """Registers the commitments leaves [k][4] as voters [n, n + k) and returns n.
        A batch that does not fit first reserves double the capacity (or what the
        batch needs); with reserve=False it is refused, as qp_registry_append does."""
        self._no_keys("append")
        a = self._leaves(leaves, first=self.size)
        first, k = self.size, a.shape[0]
        if not k:
            return first
        cap = self.capacity
        if first + k > cap:
            if not reserve:
                raise ValueError(f"{first} + {k} voters exceed the capacity {cap}; call reserve first")
            if first + k > MAX_VOTERS:
                raise ValueError(f"{first} + {k} voters are more than 2^{MAX_DEPTH}, the most the voting circuit holds")
            self.reserve(min(max(2 * cap, first + k), MAX_VOTERS))
        if self.h is None:
            self._host_append(a)
            self._epoch += 1
            return first
        self.ctx.check(lib().qp_registry_append(self.h, a.ctypes.data, k, None), "qp_registry_append")
        self._refresh()
        return first

    def replace(self, indices, leaves):
        """Replaces the commitments of voters `indices` (no index twice).  Striking a
        voter off is replacing the commitment with one nobody holds a key for."""
        self._no_keys("replace")
        idx = self._indices(indices)
        seen = {}
        for pos, i in enumerate(int(x) for x in idx):
            if i in seen:
                raise ValueError(f"voter index {i} (position {pos}) appears twice in the batch")
            seen[i] = pos
        a = self._leaves(leaves, idx=idx)
        if a.shape[0] != len(idx):
            raise ValueError(f"{a.shape[0]} commitments for {len(idx)} voters")
        if not len(idx):
            return
        if self.h is None:
            lv = self._levels
            dirty = sorted(seen)
            for i, row in zip(idx, a):
                lv[0][int(i)] = [int(x) for x in row]
            for l in range(1, len(lv)):
                dirty = sorted({i >> 1 for i in dirty})
                for j in dirty:
                    lv[l][j] = self._host_node(l, j)
            self.root = list(lv[-1][0])
            self._epoch += 1
            return
        self.ctx.check(lib().qp_registry_replace(self.h, idx.ctypes.data, a.ctypes.data, len(idx)),
                       "qp_registry_replace")
        self._refresh()

    def reserve(self, capacity):
        """Moves the tree to a layout for `capacity` >= size leaves; the root does not change."""
        self._no_keys("reserve")
        capacity = int(capacity)
        self._check_capacity(self.size, capacity)
        if self.h is None:
            if capacity != self._capacity:
                self._capacity = capacity
                self._epoch += 1
            return
        self.ctx.check(lib().qp_registry_reserve(self.h, capacity), "qp_registry_reserve")

    def level(self, l):
        """Digests [len][4] of level l (0 = the leaves, num_levels - 1 = the root)."""
        if not self.size:
            raise ValueError("the registry is empty: no voter has registered yet")
        if not 0 <= l < self.num_levels:
            raise ValueError(f"level {l} outside the tree's {self.num_levels} levels")
        if self._levels is not None:
            return np.array(self._levels[l], dtype=np.uint64).reshape(-1, 4)
        ln = ctypes.c_uint64()
        self.ctx.check(lib().qp_registry_level(self.h, l, None, ctypes.byref(ln)), "qp_registry_level")
        out = np.zeros((ln.value, 4), np.uint64)
        self.ctx.check(lib().qp_registry_level(self.h, l, out.ctypes.data, None), "qp_registry_level")
        return out

    def build_times(self):
        """Device times of the build (ms): key upload, leaf digests, levels (device registries)."""
        if self.h is None:
            raise ValueError("the host fallback has no device build times")
        ms = (ctypes.c_double * 3)()
        self.ctx.check(lib().qp_registry_build_times(self.h, ms), "qp_registry_build_times")
        return {"upload_ms": ms[0], "leaves_ms": ms[1], "levels_ms": ms[2]}

    def _indices(self, indices):
        idx = [int(i) for i in indices]
        for pos, i in enumerate(idx):
            if not 0 <= i < self.size:
                raise ValueError(f"voter index {i} (position {pos}) is outside the registry's {self.size} voters")
        return np.array(idx, dtype=np.uint64)

    def paths_raw(self, indices):
        """The dense batch buffers: siblings [B][32][4] (the zero digest from the
        depth up), path_bits [B] (bit j = side of sibling j, 1 = the voter's node
        is the right child), depth [B].  Valid under the root of the current epoch."""
        if not self.size:
            raise ValueError("the registry is empty: no voter has registered yet, so there is no path")
        idx = self._indices(indices)
        nb = len(idx)
        sib = np.zeros((nb, PATH_SLOTS, 4), np.uint64)
        bits = np.zeros(nb, np.uint32)
        depth = np.zeros(nb, np.uint32)
        if self._levels is None:
            if nb:
                self.ctx.check(lib().qp_registry_paths(self.h, idx, nb, sib, bits, depth), "qp_registry_paths")
            return sib, bits, depth
        for b, i in enumerate(int(x) for x in idx):
            d = 0
            for lv in self._levels[:-1]:
                s = i ^ 1
                if s < len(lv):  # hashed at this level; a lone last node is promoted: no sibling
                    sib[b, d] = lv[s]
                    bits[b] |= np.uint32((i & 1) << d)
                    d += 1
                i >>= 1
            depth[b] = d
        return sib, bits, depth

    def paths(self, indices):
        """(merkle_siblings, path_indices, actual_merkle_depth) per voter, as
        VotePrivateInputs takes them: lists of depth digests and depth bools."""
        sib, bits, depth = self.paths_raw(indices)
        sibs = [[[int(x) for x in sib[b, j]] for j in range(int(depth[b]))] for b in range(len(depth))]
        path = [[bool((int(bits[b]) >> j) & 1) for j in range(int(depth[b]))] for b in range(len(depth))]
        return sibs, path, [int(d) for d in depth]

    def inputs(self, index, proposal_id, vote, zk_randomness=None):
        """VoteCircuitData of voter `index` voting `vote` on `proposal_id`."""
        self._needs_keys("inputs")
        return self._vote_data([int(x) for x in self.keys[self._indices([index])[0]]], index, proposal_id, vote,
                               zk_randomness)

    def _needs_keys(self, what):
        if self.keys is None:
            raise ValueError(f"{what}: this registry was built from commitments and holds no keys; a voter builds "
                             "their inputs from their own key with inputs_for")

    def inputs_for(self, key, index, proposal_id, vote, zk_randomness=None):
        """VoteCircuitData of the voter who holds `key` and registered as `index`:
        the key is the voter's own, the path and the root are the registry's (of
        the current epoch).  What a voter's client calls; a key whose walk up
        the path does not end at the root is refused."""
        key = _digest(key, "the private key")
        data = self._vote_data(key, index, proposal_id, vote, zk_randomness)
        cur = hash_no_pad(key)
        for s, right in zip(data.private_inputs.merkle_siblings, data.private_inputs.path_indices):
            cur = hash_no_pad(list(s) + cur if right else cur + list(s))
        if cur != list(self.root):
            raise ValueError(f"the key is not the one voter {int(index)} registered: its commitment does not lead to "
                             "the registry's root")
        return data

    def _vote_data(self, key, index, proposal_id, vote, zk_randomness):
        from .synthetic import vote_nullifier
        proposal = _digest(proposal_id, "proposal_id")
        sibs, path, depth = self.paths([index])
        return VoteCircuitData(
            VotePublicInputs(proposal_id=proposal, merkle_root=list(self.root), vote=bool(vote),
                             nullifier=vote_nullifier(key, proposal)),
            VotePrivateInputs(private_key=key, merkle_siblings=sibs[0], path_indices=path[0],
                              actual_merkle_depth=depth[0]),
            zk_randomness=zk_randomness)

    def prove(self, prover, indices, proposal_id, votes):
        """One voting proof per voter of `indices` (votes: one bool, or one per
        voter) on a voting-circuit Prover; a device registry needs a prover of
        its own context."""
        self._needs_keys("prove")
        idx = self._indices(indices)
        nb = len(idx)
        if not nb:
            return []
        votes = [bool(votes)] * nb if isinstance(votes, (bool, int)) else [bool(v) for v in votes]
        if len(votes) != nb:
            raise ValueError(f"{len(votes)} votes for {nb} voters")
        proposal = _digest(proposal_id, "proposal_id")
        if self.h is None:
            return prover.prove_inputs([self.inputs(int(i), proposal, v) for i, v in zip(idx, votes)])
        arr = (_Ballot * nb)()
        for b in range(nb):
            arr[b].proposal_id[:] = proposal
            arr[b].vote = int(votes[b])
        return prover._prove(nb, "qp_prover_prove_voters",
                             lambda out, lens: lib().qp_prover_prove_voters(
                                 prover.h, self.h, idx, ctypes.cast(arr, ctypes.c_void_p), nb, out, prover.proof_size,
                                 lens))

    def free(self):
        if self.h:
            lib().qp_registry_free(self.h)
            self.h = None
        if self._own_ctx is not None:
            self._own_ctx.close()
            self._own_ctx = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
