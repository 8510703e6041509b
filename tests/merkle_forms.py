"""Which Merkle, leaf-hash and FRI-leaf kernel runs for which shape: a model of
the launchers' dispatch, and the case tables of test_gpu_merkle_forms.py (test
infrastructure).

The five thresholds (MERKLE_ROW_MAX, MERKLE_COOP_MAX, MERKLE_COOP_NBAT,
MERKLE_FUSE_LOG in csrc/merkle.hip, FRI_ROW_MAX in csrc/fri.hip) and
the widths of the fixed-width leaf kernel are read out of the sources by regular
expression; one that is not found is an error, so the numbers cannot drift.
The control flow is restated by hand: level_plan must follow merkle_tree,
leaf_form must follow leaf_hash and fri_leaf_form must follow fri_leaf, line by
line.  Whoever changes one of those launchers changes its model here.

Hooks are written as QPGPU_PATHS takes them ("key=value[,key=value...]", ""
for none).  Levels count from the leaf digests (level 0); level k of a tree of
2^log_N leaves has 2^(log_N - k) nodes.
"""
import functools
import os
import re

from test_gpu_seams import FRI_CASES as SEAM_FRI_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qp-zk-circuits-rm_amd", "csrc")
G = 0xC65C18B67785D900

CONSTANT_SOURCES = {"MERKLE_ROW_MAX": "merkle.hip", "MERKLE_COOP_MAX": "merkle.hip", "MERKLE_COOP_NBAT": "merkle.hip",
                    "MERKLE_FUSE_LOG": "merkle.hip", "FRI_ROW_MAX": "fri.hip"}


def read_constant(name, text):
    """The value of `constexpr <type> ... name = <integer>` in text; LookupError if there is none or more than one."""
    found = re.findall(r"\bconstexpr\b[^;]*?\b%s\s*=\s*(\d+)\s*[,;]" % re.escape(name), text)
    if len(found) != 1:
        raise LookupError("%s: %d definitions found, want 1" % (name, len(found)))
    return int(found[0])


def read_leaf_widths(text):
    """The column counts leaf_hash sends to k_leaf_hash_t<NC>."""
    found = re.findall(r"\bcase\s+(\d+)\s*:\s*k_leaf_hash_t<(\d+)>", text)
    if not found or any(a != b for a, b in found):
        raise LookupError("k_leaf_hash_t cases: %r" % (found,))
    return frozenset(int(a) for a, _ in found)


@functools.lru_cache(maxsize=None)
def constants():
    texts = {}
    for f in set(CONSTANT_SOURCES.values()):
        with open(os.path.join(CSRC, f)) as fh:
            texts[f] = fh.read()
    c = {name: read_constant(name, texts[f]) for name, f in CONSTANT_SOURCES.items()}
    c["LEAF_T_WIDTHS"] = read_leaf_widths(texts["merkle.hip"])
    return c


def parse_hooks(hooks):
    """path_opt's view of a QPGPU_PATHS string: {key: integer}."""
    out = {}
    for item in hooks.split(","):
        if item:
            key, value = item.split("=")
            out.setdefault(key, int(value))  # path_opt returns the first match
    return out


def level_plan(log_N, cap_h, nbat, hooks="", first_level=1):
    """The launches of merkle_tree: [(kernel, first level, levels in the
    launch, blocks per tree (grid.x), threads per block)]."""
    c, h = constants(), parse_hooks(hooks)
    K = log_N - cap_h
    row = h.get("merkle_row", 1) != 0
    coop_max = h.get("merkle_coop", c["MERKLE_ROW_MAX"] if row else c["MERKLE_COOP_MAX"])
    coop_nbat = h.get("merkle_nbat", c["MERKLE_COOP_NBAT"])
    plan, k0 = [], first_level
    while k0 <= K:
        lc = log_N - k0
        if nbat <= coop_nbat and (nbat << lc) <= coop_max:
            if row:
                plan.append(("k_merkle_level_row", k0, 1, ((1 << lc) + 15) // 16, 256))
            else:
                plan.append(("k_merkle_level_coop", k0, 1, ((1 << lc) + 3) // 4, 256))
            k0 += 1
            continue
        lb = min(lc, 8)
        nl = 1 if lc > c["MERKLE_FUSE_LOG"] else min(lb + 1, K - k0 + 1)
        plan.append(("k_merkle_level" if nl == 1 else "k_merkle_levels", k0, nl, 1 << (lc - lb), 1 << lb))
        k0 += nl
    return plan


def leaf_form(ncols, nsalt, hooks=""):
    """The kernel leaf_hash launches."""
    generic = parse_hooks(hooks).get("leaf_t", 1) == 0
    if not nsalt and not generic and ncols in constants()["LEAF_T_WIDTHS"]:
        return "k_leaf_hash_t<%d>" % ncols
    return "k_leaf_hash"


def fri_leaf_form(log_len, ab, nb, hooks=""):
    """The kernel fri_leaf launches for a layer of 2^log_len values in leaves of 2^ab."""
    lim = parse_hooks(hooks).get("fri_row", constants()["FRI_ROW_MAX"])
    nl = 1 << (log_len - ab)
    return "k_fri_leaf_row" if (2 << ab) > 4 and nl * nb <= lim else "k_fri_leaf"


# ---- trees, one batch (qp_commit_values) ---------------------------------------------------
TREE_NCOLS = 5
# (log_n, rate_bits): log N = 2, 3, 4, 5, 7, 8, 10
TREE_SHAPES = [(1, 1), (2, 1), (3, 1), (4, 1), (4, 3), (5, 3), (7, 3)]
# no hook: the row form; the wave form; the one-lane and fused forms through the
# node bound; the same through the batch bound
TREE_HOOKS = ["", "merkle_row=0", "merkle_coop=0", "merkle_nbat=0"]


def cap_heights(log_N):
    """0, 1, a middle value, log N - 1 and log N (all cap, no level)."""
    return sorted({0, 1, log_N // 2, log_N - 1, log_N})


# (log_n, rate_bits, cap height, hooks)
TREE_CASES = [(ln, rb, ch, hk) for ln, rb in TREE_SHAPES for ch in cap_heights(ln + rb) for hk in TREE_HOOKS]
# mixed plans: one-lane lower levels (512 and 256 nodes), cooperative upper levels (128 nodes down)
MIXED_CASES = [(7, 3, 0, "merkle_coop=128"), (7, 3, 0, "merkle_coop=128,merkle_row=0")]
TREE_CASES += MIXED_CASES

# ---- leaf widths ---------------------------------------------------------------------------
LEAF_SHAPE = (4, 1, 1)  # log_n, rate_bits, cap height
LEAF_WIDTHS = [1, 4, 5, 7, 8, 9, 12, 16, 17, 20, 135]
LEAF_SALTED = [4, 8, 16, 135]
LEAF_NSALT = 4
# (ncols, nsalt, hooks)
LEAF_CASES = [(w, 0, "") for w in LEAF_WIDTHS] + [(w, 0, "leaf_t=0") for w in (16, 20, 135)] + \
             [(w, LEAF_NSALT, "") for w in LEAF_SALTED]

# ---- FRI layers ----------------------------------------------------------------------------
# (nonzero coefficients log, buffer log, values log, shift, arity bits, cap height)
FRI_SHAPES = [c for c in SEAM_FRI_CASES if c[2] <= 12] + [
    (4, 4, 7, G, 2, 0),   # arity 4, 32 leaves, down to the root
    (5, 5, 8, G, 3, 0),   # arity 8, 32 leaves
    (3, 3, 6, G, 3, 1),   # arity 8, 8 leaves: half a block of rows
    (6, 8, 8, G, 4, 1),   # arity 16, 16 leaves, zero tail
    (4, 4, 6, 7, 4, 0),   # arity 16, 4 leaves
    (1, 1, 2, G, 1, 0),   # two leaves, arity 2: one node
    (2, 2, 3, G, 2, 1),   # two leaves, arity 4, all cap
    (3, 3, 5, 7, 4, 0),   # two leaves, arity 16
]
FRI_HOOKS = ["", "fri_row=0", "merkle_coop=0", "merkle_row=0", "fri_row=0,merkle_coop=0"]
FRI_FORM_CASES = [(shape, hk) for shape in FRI_SHAPES for hk in FRI_HOOKS]

# ---- the batched entry (qp_commit_values_dev) -----------------------------------------------
DEV_SHAPES = [(4, 1, 0), (4, 1, 2), (7, 3, 0)]  # log_n, rate_bits, cap height
# (batches, hooks): 33 > MERKLE_COOP_NBAT reaches the throughput forms by itself
DEV_BATCHES = [(1, ""), (3, ""), (3, "merkle_coop=0"), (3, "merkle_row=0"), (33, "")]
DEV_CASES = [(shape, nbat, hk) for shape in DEV_SHAPES for nbat, hk in DEV_BATCHES]


def all_tree_plans():
    """(case description, hooks, log N of the tree, plan) of every tree the GPU tests build."""
    out = []
    for ln, rb, ch, hk in TREE_CASES:
        out.append((("tree", ln, rb, ch), hk, ln + rb, level_plan(ln + rb, ch, 1, hk)))
    ln, rb, ch = LEAF_SHAPE
    for w, ns, hk in LEAF_CASES:
        out.append((("leaf", w, ns), hk, ln + rb, level_plan(ln + rb, ch, 1, hk)))
    for (lnz, lbuf, lv, shift, ab, ch), hk in FRI_FORM_CASES:
        out.append((("fri", lv, ab, ch), hk, lv - ab, level_plan(lv - ab, ch, 1, hk)))
    for (ln, rb, ch), nbat, hk in DEV_CASES:
        out.append((("dev", ln, rb, ch, nbat), hk, ln + rb, level_plan(ln + rb, ch, nbat, hk)))
    return out


def dev_values(shape, nbat, call):
    """[nbat][TREE_NCOLS][2^log_n] random field elements: other values for every batch and for each call."""
    import numpy as np
    log_n, rate_bits, cap_h = shape
    rng = np.random.default_rng([nbat, log_n, rate_bits, cap_h, call])
    return rng.integers(0, 0xFFFFFFFF00000001, size=(nbat, TREE_NCOLS, 1 << log_n), dtype=np.uint64)


# a handle of DEV_REFUSAL_SHAPE with 3 batches, then calls on it that differ in
# (batches, columns, log_n, rate_bits, cap height): each one other shape
DEV_REFUSAL_SHAPE = (4, 1, 2)
DEV_REFUSALS = [(2, 5, 4, 1, 2), (3, 4, 4, 1, 2), (3, 5, 3, 1, 2), (3, 5, 4, 2, 2), (3, 5, 4, 1, 1)]


def dev_child(out_path):
    """Runs DEV_CASES and the refusals through qp_commit_values_dev and saves
    what the device gave (np.savez) for the test to compare with the oracle.

    A process of its own, shaped like tools/kbench.py: torch is imported before
    the library is loaded, so both run on the HIP runtime torch ships.  In a
    process that has loaded the library first (the test process) the library
    has the system's runtime and torch cannot initialise its own beside it.
    Values go up as a torch int64 tensor viewed from uint64 numpy, the context
    runs on torch's current stream, and since that is the null stream, for
    which the context keeps its own, the device is synchronised on both sides
    of the entry, which does not synchronise itself."""
    import ctypes
    import sys

    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "qp-zk-circuits-rm_amd"))
    import qp_wormhole
    from qp_wormhole import _native
    L = _native.lib()
    ctx = qp_wormhole.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {}

    def commit(vals, rate_bits, cap_h, handle, nbat=None, null_values=False):
        npolys, n = vals.shape[1:]
        x = torch.from_numpy(np.ascontiguousarray(vals).view(np.int64)).cuda()
        cap = torch.zeros((vals.shape[0], 1 << cap_h, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = L.qp_commit_values_dev(ctx.h, None if null_values else x.data_ptr(),
                                    vals.shape[0] if nbat is None else nbat, npolys, n.bit_length() - 1, rate_bits,
                                    cap_h, cap.data_ptr(), ctypes.byref(handle))
        torch.cuda.synchronize()
        return rc, cap.cpu().numpy().view(np.uint64)

    def read(key, handle, nbat, log_n, rate_bits, cap_h, caps):
        N = 1 << (log_n + rate_bits)
        lde = np.zeros((nbat, TREE_NCOLS, N), np.uint64)           # qp_batch_lde and _coeffs copy every batch
        coeffs = np.zeros((nbat, TREE_NCOLS, 1 << log_n), np.uint64)
        leaves = np.zeros((N, TREE_NCOLS), np.uint64)              # qp_batch_open opens the first batch
        sibs = np.zeros((N, log_n + rate_bits - cap_h, 4), np.uint64)
        ok = L.qp_batch_lde(handle, lde) == 0 and L.qp_batch_coeffs(handle, coeffs) == 0 and \
            L.qp_batch_open(handle, np.arange(N, dtype=np.uint32), N, leaves, sibs) == 0
        if not ok:
            raise RuntimeError("%s: %s" % (key, L.qp_ctx_last_error(ctx.h).decode()))
        out.update({key + ".caps": caps, key + ".lde": lde, key + ".coeffs": coeffs, key + ".leaves": leaves,
                    key + ".sibs": sibs})

    for i, (shape, nbat, hooks) in enumerate(DEV_CASES):
        log_n, rate_bits, cap_h = shape
        os.environ.pop("QPGPU_PATHS", None)
        if hooks:
            os.environ["QPGPU_PATHS"] = hooks
        h = ctypes.c_void_p()
        try:
            for call in range(2):  # the second call reuses the handle on new values
                before = h.value
                rc, caps = commit(dev_values(shape, nbat, call), rate_bits, cap_h, h)
                if rc or not h.value or (call and h.value != before):
                    raise RuntimeError("case %d call %d: status %d, handle %r after %r, %s" % (
                        i, call, rc, h.value, before, L.qp_ctx_last_error(ctx.h).decode()))
                read("%d.%d" % (i, call), h, nbat, log_n, rate_bits, cap_h, caps)
        finally:
            L.qp_batch_free(h)
    os.environ.pop("QPGPU_PATHS", None)

    log_n, rate_bits, cap_h = DEV_REFUSAL_SHAPE
    vals = dev_values(DEV_REFUSAL_SHAPE, 3, 0)
    h = ctypes.c_void_p()
    try:
        rc, caps = commit(vals, rate_bits, cap_h, h)
        if rc:
            raise RuntimeError("refusals: rc %d, %s" % (rc, L.qp_ctx_last_error(ctx.h).decode()))
        kept, rcs, errs, same = h.value, [], [], []
        for nb, nc, ln, rb, ch in DEV_REFUSALS:
            rc, _ = commit(vals[:nb, :nc, :1 << ln], rb, ch, h)
            rcs.append(rc)
            errs.append(L.qp_ctx_last_error(ctx.h).decode())
            same.append(h.value == kept)
        out.update({"refuse.rc": np.array(rcs), "refuse.err": np.array(errs), "refuse.kept": np.array(same)})
        rc, caps = commit(vals, rate_bits, cap_h, h)  # and it still serves its own shape
        if rc:
            raise RuntimeError("after the refusals: rc %d, %s" % (rc, L.qp_ctx_last_error(ctx.h).decode()))
        read("refuse.after", h, 3, log_n, rate_bits, cap_h, caps)
    finally:
        L.qp_batch_free(h)
    fresh = ctypes.c_void_p()
    try:
        rc0, caps0 = commit(vals, rate_bits, cap_h, fresh, nbat=0)
        made0 = bool(fresh.value)
        rc1, caps1 = commit(vals, rate_bits, cap_h, fresh, null_values=True)
        out.update({"null.rc": np.array([rc0, rc1]), "null.handle": np.array([made0, bool(fresh.value)]),
                    "null.caps_written": np.array([bool(caps0.any()), bool(caps1.any())])})
    finally:
        L.qp_batch_free(fresh)
    torch.cuda.synchronize()
    ctx.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    import sys
    dev_child(sys.argv[1])
