"""The transfer ledger's log commitment, receipts and log audit on the device
(csrc/ledger.hip: k_ledger_leaves, k_ledger_gather, k_ledger_audit_screen,
k_ledger_audit_resolve, k_ledger_audit_payouts; the levels, paths and prefix
roots through the accumulator tree's launchers): the cases of
test_ledger_log.py against the same model and, result for result, against the
host path; the leaf kernel's block edges; the ledger's tree against a registry
built from its leaves; then real Wormhole proofs end to end."""
import ctypes

import numpy as np
import pytest

from ledger_log_model import (OK, PAYOUTS, SIZES, LedgerLogModel, audit, check_big_totals, check_counted_double_spend,
                              check_honest_stream, check_leaf_edges, check_receipt_rules, check_roots_at_every_m,
                              check_size, check_tamperings, leaf, log_of, payouts_claim, run_commit_stream, same,
                              sized_items)
from ledger_model import ROOT_A, STREAMS, Model, cast_batch, make_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_ledger(ctx):
    from qp_wormhole import WormholeLedger
    return lambda roots, padding, cap: WormholeLedger(ctx, roots, padding=padding, capacity=cap)


def host_ledger(roots, padding, capacity):
    from qp_wormhole import WormholeLedger
    return WormholeLedger(None, roots, padding=padding, capacity=capacity)


@pytest.mark.parametrize("name", STREAMS)
def test_root_matches_model_and_host_path(device_ledger, name):
    """batchings 7 and whole commit after every batch, 64 once at the end; the final commitment and the
    receipts of the first, a middle and the last entry are equal across the three and equal to the host path's"""
    finals = [run_commit_stream(device_ledger, name, batching, every)
              for batching, every in ((7, True), (None, True), (64, False))]
    assert finals[0] == finals[1] == finals[2] == run_commit_stream(host_ledger, name, 64, False)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_promoted_nodes(device_ledger, n):
    assert check_size(device_ledger, n) == check_size(host_ledger, n)


def test_leaf_edge_values(device_ledger):
    assert check_leaf_edges(device_ledger) == check_leaf_edges(host_ledger)


def test_receipt_rules(device_ledger):
    assert check_receipt_rules(device_ledger) == check_receipt_rules(host_ledger)


def test_roots_at_every_m(device_ledger):
    assert check_roots_at_every_m(device_ledger) == check_roots_at_every_m(host_ledger)


def test_leaf_kernel_block_edges(device_ledger):
    """257 entries in one batch and one commit (two blocks, the second with one lane); then commits at
    7, 256 and 300 entries, so the leaf launches start at 0, 7 and 256 and end ragged.  Every root is
    the model's."""
    items = sized_items(300, seed=300)
    for cuts in ([257], [7, 256, 300]):
        model, logm = Model([ROOT_A]), LedgerLogModel()
        led = device_ledger([ROOT_A], None, 300)
        try:
            done = 0
            for n in cuts:
                cast_batch(led, items[done:n])
                for pi, v in items[done:n]:
                    model.cast_one(pi, v)
                logm.sync(model)
                done = n
                assert led.commit_log() == (logm.root(n), n), (cuts, n)
            assert led.roots_at(cuts) == [logm.root(n) for n in cuts]
        finally:
            led.free()


@pytest.mark.parametrize("hook", [None, "registry_row=0"], ids=["default", "one_lane"])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 129])
def test_one_tree_serves_ledger_and_registry(ctx, device_ledger, monkeypatch, hook, n):
    """The ledger's log is the third client of the accumulator tree (csrc/acc_tree.h): a commitment
    registry built from the committed ledger's model leaves has the ledger's root, and its paths_raw are
    the receipts' buffers bit for bit.  Sizes: no parent, one pair, a promoted leaf, ACC_FOLD_MAX = 64 on
    the leaf level (64, 65) and on the level above (129).  Every fourth entry is a double spend.  With
    the one-lane form (registry_row=0) and the default, which governs both trees."""
    from qp_wormhole import VoterRegistry
    from qp_wormhole._native import lib
    from qp_wormhole.ledger import PATH_SLOTS
    if hook:
        monkeypatch.setenv("QPGPU_PATHS", hook)
    else:
        monkeypatch.delenv("QPGPU_PATHS", raising=False)
    items = sized_items(n, seed=1000 + n)
    doubles = [i for i in range(n) if i % 4 == 1]
    for i in doubles:
        items[i] = (items[i - 1][0][0:4] + items[i][0][4:], 0)
    model = Model([ROOT_A])
    led = device_ledger([ROOT_A], None, n)
    reg = None
    try:
        cast_batch(led, items)
        for pi, v in items:
            model.cast_one(pi, v)
        assert [i for i, e in enumerate(model.log) if not e[4]] == doubles
        root, committed = led.commit_log()
        assert committed == n == led.admitted
        leaves = [leaf(e) for e in model.log]
        reg = VoterRegistry.from_commitments(ctx, leaves)
        assert [int(x) for x in reg.root] == root
        seqs = np.array(sorted({0, n // 2, n - 1}), dtype=np.uint64)
        k = len(seqs)
        sib, bits, depth = reg.paths_raw(seqs)
        rsib = np.full((k, PATH_SLOTS, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)  # every slot is written
        rbits, rdepth = np.full(k, 0xFFFFFFFF, np.uint32), np.full(k, 0xFFFFFFFF, np.uint32)
        rleaf, rroot, rn = np.zeros((k, 4), np.uint64), np.zeros(4, np.uint64), ctypes.c_uint64()
        assert lib().qp_ledger_receipts(led.h, seqs.ctypes.data, k, rsib.ctypes.data, rbits.ctypes.data,
                                        rdepth.ctypes.data, rleaf.ctypes.data, rroot.ctypes.data, ctypes.byref(rn)) == 0
        assert (rroot.tolist(), rn.value) == (root, n)
        assert rsib.tobytes() == sib.tobytes() and rbits.tobytes() == bits.tobytes()
        assert rdepth.tobytes() == depth.tobytes()
        assert rleaf.tolist() == [leaves[int(s)] for s in seqs]
    finally:
        if reg is not None:
            reg.free()
        led.free()


@pytest.mark.parametrize("name", STREAMS + ["runs_513_3"])
def test_audit_honest_streams(ctx, device_ledger, name):
    assert check_honest_stream(ctx, device_ledger, name) == check_honest_stream(None, host_ledger, name)


def test_audit_tamperings(ctx, device_ledger):
    assert check_tamperings(ctx, device_ledger) == check_tamperings(None, host_ledger)


def test_audit_counted_double_spend(ctx, device_ledger):
    assert check_counted_double_spend(ctx, device_ledger) == check_counted_double_spend(None, host_ledger)


def test_audit_totals_beyond_2_128(ctx, device_ledger):
    assert check_big_totals(ctx, device_ledger) == check_big_totals(None, host_ledger)


def test_device_audit_of_a_host_log_and_back(ctx, device_ledger):
    """the paths publish the same log, and each audits the other's"""
    from qp_wormhole import audit_ledger_log
    cap, roots, padding, items = make_stream("grow")
    published = []
    for factory in (device_ledger, host_ledger):
        led = factory(roots, padding, 128)
        try:
            cast_batch(led, [it for it in items if it[0] != "reserve"])
            published.append((led.entries(), led.commit_log(), led.payouts(), led.recount()))
        finally:
            led.free()
    (ed, cd, pd, rd), (eh, ch, ph, rh) = published
    assert (cd, pd, rd) == (ch, ph, rh) and all((a == b).all() if hasattr(a, "all") else a == b for a, b in zip(ed, eh))
    for c, entries in ((ctx, eh), (None, ed)):
        rep = audit_ledger_log(c, entries, root=cd[0], totals=(rd[0], rd[2]), payouts=pd, commitments=[cd])
        same(rep, audit(log_of(entries), cd[0], (rd[0], rd[2]), payouts_claim(pd), [cd]))
        assert rep.status == OK


def test_wormhole_proofs_to_receipts_and_audit(ctx):
    import qp_wormhole
    from qp_wormhole import WormholeLedger, WormholeVerifier, audit_ledger_log
    from qp_wormhole.synthetic import synthetic_inputs
    config = "standard_recursion_zk_config"
    proofs = [qp_wormhole.WormholeProver(config).commit(synthetic_inputs(40 + k, k % 3)).prove() for k in range(3)]
    pis = [[int(x) for x in p.public_inputs] for p in proofs]
    ver = WormholeVerifier(config)
    led = None
    try:
        batch = [p.to_bytes() for p in proofs] + [proofs[1].to_bytes()]  # the last one a double spend
        led = WormholeLedger(ctx, [pi[4:8] for pi in pis], verifier=ver)
        assert [r.status for r in led.cast(batch)] == [0, 0, 0, 6]
        root, n = led.commit_log()
        assert n == led.admitted == 4
        # each exit account's owner reads the nullifier from the proof itself: the 16 public inputs are its last 128 bytes
        nuls = [np.frombuffer(bytes(b)[-128:], "<u8")[0:4].tolist() for b in batch]
        assert nuls[:3] == [pi[0:4] for pi in pis] and nuls[3] == nuls[1]
        for i in range(3):
            r = led.receipt_for(nuls[i])
            assert (r.seq, r.number, r.credited, r.amount, r.account) == (i, i, True, pis[i][8:12], pis[i][12:16])
            assert (r.root, r.n) == (root, n) and WormholeLedger.check_receipt(r, root, n)
        assert led.receipt_for(nuls[3]).seq == 1  # the double spend's nullifier gives the credited entry
        second = led.receipts([3])[0]
        assert (second.number, second.credited) == (3, False) and WormholeLedger.check_receipt(second, root, n)
        assert led.receipt_for([1, 2, 3, 4]) is None
        # what the settler publishes, audited by a third party
        entries, payouts = led.entries(), led.payouts()
        credited, _, total = led.recount()
        earlier = [(led.root_at(2), 2)]
        rep = audit_ledger_log(ctx, entries, root, (credited, total), payouts, earlier)
        assert (rep.status, rep.root, rep.credited, rep.total, rep.accounts) == (OK, root, 3, total, len(payouts))
        assert rep == audit_ledger_log(None, entries, root, (credited, total), payouts, earlier)
        cheat = [(payouts[0][0], payouts[0][1] + 1, payouts[0][2])] + payouts[1:]
        bad = audit_ledger_log(ctx, entries, root, (credited, total), cheat, earlier)
        assert (bad.status, bad.witness) == (PAYOUTS, 0)
    finally:
        if led is not None:
            led.free()
        ver.close()
