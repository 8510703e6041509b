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
"""
import ctypes

import numpy as np

from ._native import Context, hash_no_pad, lib
from .circuits import U64_4, VoteCircuitData, VotePrivateInputs, VotePublicInputs

P = 0xFFFFFFFF00000001
PATH_SLOTS = 32          # MAX_MERKLE_DEPTH (voting/src/lib.rs:20)
MAX_DEPTH = 31           # depth 32 does not fit the circuit's 5-bit depth split
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
        self.keys, self.size = k, n
        self.max_depth = (n - 1).bit_length()
        self.num_levels = self.max_depth + 1
        self.h = self._levels = self._own_ctx = None
        if ctx_or_device is None:
            self.ctx = None
            self._build_host()
        else:
            if isinstance(ctx_or_device, Context):
                self.ctx = ctx_or_device
            else:
                self.ctx = self._own_ctx = Context(int(ctx_or_device))
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

    def level(self, l):
        """Digests [len][4] of level l (0 = the leaves, num_levels - 1 = the root)."""
        if not 0 <= l < self.num_levels:
            raise ValueError(f"level {l} outside the tree's {self.num_levels} levels")
        if self._levels is not None:
            return self._levels[l]
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
        is the right child), depth [B]."""
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
        from .synthetic import vote_nullifier
        proposal = _digest(proposal_id, "proposal_id")
        sibs, path, depth = self.paths([index])
        key = [int(x) for x in self.keys[int(index)]]
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
