"""Every form of the Merkle level, leaf-hash and FRI-leaf kernels at small
shapes, bit-exact against the CPU oracle (oracle/merkle.c, which shares no code
with the device).

csrc/merkle.hip has four level kernels (k_merkle_level, k_merkle_levels,
k_merkle_level_coop, k_merkle_level_row) and two leaf kernels (k_leaf_hash,
k_leaf_hash_t<135|20|16>); csrc/fri.hip has k_fri_leaf and
k_fri_leaf_row.  The launchers choose by nodes x batch, and at batch 1 every
small tree takes the row form, so the path hooks of csrc/paths.h force the
others.  merkle_forms.py models that choice; the tests without a gpu mark check
on the model that the case tables reach each kernel at each of its edges (a
narrow block, several blocks, every fused level count, rows and waves past a
level's end, no level at all), and the gpu tests then run the tables.

Every tree is opened at every leaf: the siblings of all leaves are all nodes of
all levels below the cap, so a mismatch names its level.

qp_commit_values_dev, the batched commit of the C ABI, takes device pointers.
Its cases run in one child process (merkle_forms.dev_child), which puts the
values on the device through torch; the tests compare what it read back.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import merkle_forms as mf
from edge_values import constant_columns, edge_cycle
from oracle_lib import P, commit_values, lib as olib


def rand_felts(rng, *shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def hooks_id(hooks):
    return hooks or "nohook"


def nodes(log_N, launch):
    return 1 << (log_N - launch[1])


# ---- the dispatch model and the reach of the case tables: no GPU ---------------------------

def test_thresholds_are_read_from_the_sources():
    c = mf.constants()
    for name in mf.CONSTANT_SOURCES:
        assert isinstance(c[name], int) and c[name] > 0, name
    assert c["LEAF_T_WIDTHS"] == {135, 20, 16}
    with pytest.raises(LookupError):
        mf.read_constant("MERKLE_NO_SUCH_BOUND", "constexpr long MERKLE_ROW_MAX = 32768;")
    with pytest.raises(LookupError):
        mf.read_constant("MERKLE_ROW_MAX", "// MERKLE_ROW_MAX = 32768 nodes")
    assert mf.read_constant("B", "constexpr long A = 1, B = 22, C = 3;") == 22
    with pytest.raises(LookupError):
        mf.read_leaf_widths("switch (ncols) { default: break; }")


def test_plans_cover_every_level_once():
    for case, hooks, log_N, plan in mf.all_tree_plans():
        cap_h = case[3] if case[0] in ("tree", "fri", "dev") else mf.LEAF_SHAPE[2]
        want = 1
        for name, k0, nl, blocks, threads in plan:
            assert k0 == want and nl >= 1, (case, hooks, plan)
            if name in ("k_merkle_level", "k_merkle_levels"):  # one lane per node of the launch's first level
                assert blocks * threads == nodes(log_N, (name, k0)), (case, hooks, plan)
            want = k0 + nl
        assert want == log_N - cap_h + 1, (case, hooks, plan)


def test_one_batch_without_a_hook_is_the_row_form_only():
    """The gap these tests close: the heuristic alone shows a one-batch small tree one kernel."""
    for case, hooks, log_N, plan in mf.all_tree_plans():
        if not hooks and case[0] != "dev":
            assert {launch[0] for launch in plan} <= {"k_merkle_level_row"}, (case, plan)


def launches(kernel, want_hooks=None):
    return [(case, hooks, log_N, launch) for case, hooks, log_N, plan in mf.all_tree_plans() for launch in plan
            if launch[0] == kernel and (want_hooks is None or hooks == want_hooks)]


def test_tables_reach_the_one_lane_level_kernel():
    got = launches("k_merkle_level")
    assert any(blocks > 1 and threads == 256 for _, _, _, (_, _, _, blocks, threads) in got)
    assert any(blocks == 1 and threads == 256 for _, _, _, (_, _, _, blocks, threads) in got)
    assert any(blocks == 1 and threads < 256 for _, _, _, (_, _, _, blocks, threads) in got)
    assert all(nl == 1 for _, _, _, (_, _, nl, _, _) in got)
    # through each of the two conditions, and by the heuristic alone
    for hooks in ("merkle_coop=0", "merkle_nbat=0", ""):
        assert launches("k_merkle_level", hooks), hooks


def test_tables_reach_every_fused_level_count():
    got = launches("k_merkle_levels")
    by_cap, by_block = set(), set()
    for case, hooks, log_N, (_, k0, nl, blocks, threads) in got:
        lb = threads.bit_length() - 1
        assert blocks == 1 and threads == nodes(log_N, (None, k0)) and 2 <= nl <= lb + 1
        (by_block if nl == lb + 1 else by_cap).add(nl)
    assert by_cap | by_block == set(range(2, 8)), (by_cap, by_block)
    assert by_cap and by_block
    # a count below lb + 1 is the cap's doing: min(lb + 1, K - k0 + 1) took its second argument
    assert {2, 3, 4, 5, 6} <= by_cap and 7 in by_block
    for hooks in ("merkle_coop=0", "merkle_nbat=0", ""):
        assert launches("k_merkle_levels", hooks), hooks


def test_tables_reach_rows_and_waves_past_a_level_end():
    row = [nodes(log_N, launch) for _, _, log_N, launch in launches("k_merkle_level_row")]
    assert any(n < 16 for n in row) and any(n > 16 for n in row) and 1 in row
    coop = [nodes(log_N, launch) for _, _, log_N, launch in launches("k_merkle_level_coop")]
    assert any(n < 4 for n in coop) and any(n > 4 for n in coop) and 1 in coop
    for n, (_, _, _, (name, _, _, blocks, threads)) in zip(row, launches("k_merkle_level_row")):
        assert (blocks - 1) * 16 < n <= blocks * 16 and threads == 256
    for n, (_, _, _, (name, _, _, blocks, threads)) in zip(coop, launches("k_merkle_level_coop")):
        assert (blocks - 1) * 4 < n <= blocks * 4 and threads == 256


def test_tables_reach_the_whole_tree_shapes():
    plans = mf.all_tree_plans()
    for table in ("tree", "fri", "dev"):
        sizes = {len(plan) for case, _, _, plan in plans if case[0] == table}
        assert 1 in sizes, table
    assert 0 in {len(plan) for case, _, _, plan in plans if case[0] in ("tree", "fri")}  # cap height = log N
    assert any(sum(nl for _, _, nl, _, _ in plan) == 1 for case, _, _, plan in plans if case[0] == "tree")
    # mixed: one-lane lower levels, then cooperative upper levels
    assert (7, 3, 0, "merkle_coop=128") in mf.MIXED_CASES
    for ln, rb, ch, hooks in mf.MIXED_CASES:
        names = [launch[0] for launch in mf.level_plan(ln + rb, ch, 1, hooks)]
        upper = "k_merkle_level_coop" if "merkle_row=0" in hooks else "k_merkle_level_row"
        assert names == ["k_merkle_level"] * 2 + [upper] * 8, names
    # the throughput forms with no hook: batch 33 > MERKLE_COOP_NBAT
    assert mf.constants()["MERKLE_COOP_NBAT"] < 33
    big = [plan for case, hooks, _, plan in plans if case[0] == "dev" and case[4] == 33 and not hooks]
    assert len(big) == len(mf.DEV_SHAPES)
    for plan in big:
        assert {launch[0] for launch in plan} <= {"k_merkle_level", "k_merkle_levels"}
    assert {launch[0] for plan in big for launch in plan} == {"k_merkle_level", "k_merkle_levels"}
    # batches of 1 and 3 take the cooperative forms unless a hook says otherwise
    for case, hooks, _, plan in plans:
        if case[0] == "dev" and case[4] < 33 and not hooks:
            assert {launch[0] for launch in plan} == {"k_merkle_level_row"}


def test_tables_reach_both_leaf_kernels_at_each_fixed_width():
    forms = {(w, mf.leaf_form(w, ns, hooks)) for w, ns, hooks in mf.LEAF_CASES}
    for w in (135, 20, 16):
        assert (w, "k_leaf_hash_t<%d>" % w) in forms and (w, "k_leaf_hash") in forms
    for w, ns, hooks in mf.LEAF_CASES:
        if w not in (135, 20, 16) or ns:
            assert mf.leaf_form(w, ns, hooks) == "k_leaf_hash"
    # the batched entry's and the trees' five columns: the any-width kernel
    assert mf.leaf_form(mf.TREE_NCOLS, 0) == "k_leaf_hash"


def test_tables_reach_both_fri_leaf_kernels_at_each_arity():
    forms = {(ab, mf.fri_leaf_form(lv, ab, 1, hooks)) for (_, _, lv, _, ab, _), hooks in mf.FRI_FORM_CASES}
    for ab in (2, 3, 4):
        assert (ab, "k_fri_leaf_row") in forms and (ab, "k_fri_leaf") in forms
    # arity 2 is a leaf of four words: hash_or_noop, the one-lane kernel whatever the hook
    assert (1, "k_fri_leaf") in forms and (1, "k_fri_leaf_row") not in forms
    assert any(lv - ab == 1 for (_, _, lv, _, ab, _), _ in mf.FRI_FORM_CASES)  # a layer of two leaves
    for shape in mf.FRI_SHAPES:  # small: every leaf is opened
        assert shape[2] <= (12 if shape in mf.SEAM_FRI_CASES else 8)


# ---- on the device -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


def set_hooks(monkeypatch, hooks):
    """QPGPU_PATHS for the calls that follow (the library reads it per call)."""
    if hooks:
        monkeypatch.setenv("QPGPU_PATHS", hooks)
    else:
        monkeypatch.delenv("QPGPU_PATHS", raising=False)


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def merkle_oracle(leaves, log_N, cap_h):
    """(cap, siblings [N][depth][4]) of the oracle's tree over leaves [N][W], every leaf proven."""
    N, depth = 1 << log_N, log_N - cap_h
    cap = np.zeros((1 << cap_h, 4), np.uint64)
    sibs = np.zeros((N, max(depth, 1), 4), np.uint64)
    assert olib().ora_merkle(np.ascontiguousarray(leaves), log_N, leaves.shape[1], cap_h, cap,
                             np.arange(N, dtype=np.uint64), N, sibs) == 0
    return cap, sibs[:, :depth]


@functools.lru_cache(maxsize=None)
def commit_oracle(ncols, nsalt, log_n, rate_bits, cap_h, kind):
    """One input set per (shape, kind) and the oracle's commitment to it, shared
    by every hook of that shape: (values, salt, coeffs, leaves, cap, siblings)."""
    n, N = 1 << log_n, 1 << (log_n + rate_bits)
    if kind == "random":
        rng = np.random.default_rng(ncols * 10000 + nsalt * 1000 + log_n * 10 + rate_bits)  # not the cap: the same tree
        vals = rand_felts(rng, ncols, n)
        salt = rand_felts(rng, N, nsalt) if nsalt else None
    else:  # every column constant at a canonical edge value, so every leaf word is one
        vals = constant_columns(ncols, n, start=ncols)
        salt = edge_cycle(N * nsalt, start=3).reshape(N, nsalt) if nsalt else None
    coeffs, leaves, cap = commit_values(vals, log_n, rate_bits, cap_h, salt=salt, want_leaves=True)
    cap2, sibs = merkle_oracle(leaves, log_n + rate_bits, cap_h)
    assert (cap2 == cap).all()
    if kind == "edge":
        assert (leaves[:, :ncols] == vals[:, 0]).all()
    return frozen(vals, salt, coeffs, leaves, cap, sibs)


def check_siblings(got, want, what):
    """got/want [N][depth][4]: sibling j of a leaf is a node of level j (0 = the leaf digests)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, "%s: %d wrong nodes, the first at level %d (sibling of leaf %d); wrong levels %s" % (
        what, len(bad), bad[0][1], bad[0][0], sorted(set(int(j) for j in bad[:, 1])))


def commit_and_check(ctx, ncols, nsalt, log_n, rate_bits, cap_h, kind, what):
    """qp_commit_values against the oracle: coefficients, LDE, cap, every leaf and every node."""
    import qp_wormhole
    vals, salt, coeffs_o, leaves_o, cap_o, sib_o = commit_oracle(ncols, nsalt, log_n, rate_bits, cap_h, kind)
    N = 1 << (log_n + rate_bits)
    b = qp_wormhole.PolynomialBatch.from_values(ctx, vals, rate_bits, cap_h, salt=salt)
    try:
        assert (b.coeffs == coeffs_o).all(), (what, "coeffs")
        assert (b.lde() == leaves_o[:, :ncols].T).all(), (what, "lde")
        leaves, sibs = b.open(np.arange(N, dtype=np.uint32))
        assert (leaves == leaves_o).all(), (what, "leaves")
        check_siblings(sibs, sib_o, what)
        assert (b.cap == cap_o).all(), (what, "cap: level %d" % (log_n + rate_bits - cap_h),
                                        np.argwhere(b.cap != cap_o)[:4])
    finally:
        b.free()
    return b.cap, sibs


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,rate_bits,cap_h,hooks", mf.TREE_CASES,
                         ids=["N%d-cap%d-%s" % (ln + rb, ch, hooks_id(hk)) for ln, rb, ch, hk in mf.TREE_CASES])
def test_tree_forms(ctx, monkeypatch, log_n, rate_bits, cap_h, hooks):
    """Five columns, log N from 2 to 10, cap heights 0, 1, middle, log N - 1 and
    log N, under each form of the level kernels; random and edge-valued leaves."""
    set_hooks(monkeypatch, hooks)
    for kind in ("random", "edge"):
        commit_and_check(ctx, mf.TREE_NCOLS, 0, log_n, rate_bits, cap_h, kind, (kind, hooks))


@pytest.mark.gpu
@pytest.mark.parametrize("ncols,nsalt", sorted({(w, ns) for w, ns, _ in mf.LEAF_CASES}))
def test_leaf_widths(ctx, monkeypatch, ncols, nsalt):
    """Leaves of 1 to 139 words.  A width that is no multiple of 8 leaves the
    previous block's words in the rest of the rate (the overwrite-mode sponge of
    hash_n_to_m_no_pad): 7, 9, 12 and 17 pin that.  4 and 8 columns with 4 salt
    columns cross the no-op and the single-absorb bounds.  16, 20 and 135 run the
    fixed-width kernel and, under leaf_t=0, the any-width one: the same bytes."""
    log_n, rate_bits, cap_h = mf.LEAF_SHAPE
    for kind in ("random", "edge"):
        got = {}
        for hooks in [hk for w, ns, hk in mf.LEAF_CASES if (w, ns) == (ncols, nsalt)]:
            set_hooks(monkeypatch, hooks)
            got[hooks] = commit_and_check(ctx, ncols, nsalt, log_n, rate_bits, cap_h, kind, (kind, hooks))
        if not nsalt and ncols in (16, 20, 135):
            assert set(got) == {"", "leaf_t=0"}
            assert (got[""][0] == got["leaf_t=0"][0]).all() and (got[""][1] == got["leaf_t=0"][1]).all()


@functools.lru_cache(maxsize=None)
def fri_oracle(shape):
    lnz, lbuf, lv, shift, ab, cap_h = shape
    rng = np.random.default_rng(lnz * 100 + lv * 10 + ab)
    coeffs = np.zeros((2, 1 << lbuf), np.uint64)
    coeffs[:, :1 << lnz] = rand_felts(rng, 2, 1 << lnz)
    nleaves, depth = 1 << (lv - ab), lv - ab - cap_h
    idx = np.arange(nleaves, dtype=np.uint32)
    cap = np.zeros((1 << cap_h, 4), np.uint64)
    evals = np.zeros((nleaves, 2 << ab), np.uint64)
    sibs = np.zeros((nleaves, max(depth, 1) * 4), np.uint64)
    assert olib().ora_fri_layer(np.ascontiguousarray(coeffs), lbuf, lv, shift, ab, cap_h, cap, idx, nleaves,
                                evals, sibs) == 0
    return frozen(coeffs, idx, cap, evals, sibs[:, :depth * 4].reshape(nleaves, depth, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,hooks", mf.FRI_FORM_CASES,
                         ids=["v%d-a%d-cap%d-%s" % (s[2], s[4], s[5], hooks_id(hk)) for s, hk in mf.FRI_FORM_CASES])
def test_fri_layer_forms(ctx, monkeypatch, shape, hooks):
    """qp_fri_layer_commit at arities 2 to 16, from two leaves up, under both
    FRI leaf kernels and each form of the level kernels; every leaf opened.
    (A layer of two leaves is accepted: log_values - arity_bits = 1.)"""
    import qp_wormhole
    lnz, lbuf, lv, shift, ab, cap_h = shape
    coeffs, idx, cap_o, evals_o, sib_o = fri_oracle(shape)
    set_hooks(monkeypatch, hooks)
    layer = qp_wormhole.FriLayer(ctx, coeffs, lv, shift, ab, cap_h)
    try:
        evals, sibs = layer.open(idx)
        assert (evals.reshape(len(idx), -1) == evals_o).all(), "evaluations"
        check_siblings(sibs, sib_o, hooks)
        assert (layer.cap == cap_o).all(), ("cap: level %d" % (lv - ab - cap_h), np.argwhere(layer.cap != cap_o)[:4])
    finally:
        layer.free()


# ---- the batched entry ---------------------------------------------------------------------

QP_ERR_ARG = 1


@pytest.fixture(scope="module")
def dev_results(tmp_path_factory):
    """What merkle_forms.dev_child read back from qp_commit_values_dev, for
    every case at once: one child process, because the values have to be torch
    tensors and torch shares a process with the library only when it is
    imported first (see dev_child).  Its start (importing torch, a second
    context) is the one slow step of this module."""
    out = tmp_path_factory.mktemp("dev") / "dev.npz"
    env = {k: v for k, v in os.environ.items() if k != "QPGPU_PATHS"}
    r = subprocess.run([sys.executable, mf.__file__, str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def check_dev_batches(got, key, vals, rate_bits, cap_h):
    """Every batch of one qp_commit_values_dev call against the oracle's
    commitment to that batch's values; the first batch's opening of every leaf."""
    nbat, npolys, n = vals.shape
    log_n = n.bit_length() - 1
    caps, lde, coeffs = got[key + ".caps"], got[key + ".lde"], got[key + ".coeffs"]
    assert caps.shape == (nbat, 1 << cap_h, 4) and lde.shape[0] == nbat and coeffs.shape == vals.shape
    if nbat > 1:
        assert len({caps[bi].tobytes() for bi in range(nbat)}) == nbat, key  # other values, other caps
    for bi in range(nbat):
        coeffs_o, leaves_o, cap_o = commit_values(vals[bi], log_n, rate_bits, cap_h, want_leaves=True)
        assert (coeffs[bi] == coeffs_o).all(), (key, "coeffs", bi)
        assert (lde[bi] == leaves_o.T).all(), (key, "lde", bi)
        assert (caps[bi] == cap_o).all(), (key, "cap", bi, np.argwhere(caps[bi] != cap_o)[:4])
        if bi == 0:
            cap0, sib_o = merkle_oracle(leaves_o, log_n + rate_bits, cap_h)
            assert (cap0 == cap_o).all()
            assert (got[key + ".leaves"] == leaves_o).all(), (key, "leaves")
            check_siblings(got[key + ".sibs"], sib_o, key)


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(len(mf.DEV_CASES)),
                         ids=["n%d-r%d-cap%d-b%d-%s" % (s + (nb, hooks_id(hk))) for s, nb, hk in mf.DEV_CASES])
def test_commit_values_dev(dev_results, index):
    """The batched commit of the C ABI: batch strides, per-batch caps, the
    reused handle.  Each batch has its own values; with cap height 0 the cap is
    the root, so every node of every batch is behind the comparison.  Batches
    of 33 take the one-lane and fused level kernels by the heuristic alone,
    batches of 3 under merkle_coop=0 by the hook; merkle_row=0 gives the wave
    form.  The second call reuses the handle on new values."""
    shape, nbat, hooks = mf.DEV_CASES[index]
    for call in range(2):
        vals = mf.dev_values(shape, nbat, call)
        check_dev_batches(dev_results, "%d.%d" % (index, call), vals, shape[1], shape[2])
    assert (dev_results["%d.0.caps" % index] != dev_results["%d.1.caps" % index]).any()


@pytest.mark.gpu
def test_commit_values_dev_refusals(dev_results):
    """A handle of another shape (batches, columns, size, rate, cap height), no
    batch and no values are QP_ERR_ARG; a refused call makes no handle, writes
    no cap and leaves the handle it was given as it was."""
    got = dev_results
    assert len(got["refuse.rc"]) == len(mf.DEV_REFUSALS)
    assert (got["refuse.rc"] == QP_ERR_ARG).all() and got["refuse.kept"].all()
    assert [str(e) for e in got["refuse.err"]] == ["reused batch handle has a different shape"] * len(mf.DEV_REFUSALS)
    log_n, rate_bits, cap_h = mf.DEV_REFUSAL_SHAPE
    check_dev_batches(got, "refuse.after", mf.dev_values(mf.DEV_REFUSAL_SHAPE, 3, 0), rate_bits, cap_h)
    assert (got["null.rc"] == QP_ERR_ARG).all()  # nbat == 0, then a null values pointer
    assert not got["null.handle"].any() and not got["null.caps_written"].any()
