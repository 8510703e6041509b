"""The input screen on the device (csrc/input_screen.hip: k_screen_nodes,
k_screen_resolve) and the prove call built on it: device == host path == model
on every case of wormhole_screen_model.py, as exact integers; batches whose
lanes cross wave, block and upload-chunk edges against the host path; the screen
pinned to the circuit, no case left out, through the unchanged prove_inputs and
WormholeVerifier; Prover.prove_inputs(on_bad="skip") at the batch seam and on
all-good and all-bad batches."""
import pytest

from wormhole_screen_model import CASE_IDS, CASES, NULLIFIER, OK, mixed_batch, model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import qp_wormhole
    c = qp_wormhole.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def circuit():
    import qp_wormhole
    return qp_wormhole.Circuit.wormhole()


@pytest.fixture(scope="module")
def prover(ctx, circuit):
    """max_batch 4: the skip tests need a batch seam inside nine inputs"""
    import qp_wormhole
    p = qp_wormhole.Prover(ctx, circuit, max_batch=4)
    yield p
    p.free()


@pytest.fixture(scope="module")
def device_statuses(ctx):
    """the device path's verdicts on the whole table, one call"""
    import qp_wormhole
    return [tuple(s) for s in qp_wormhole.screen_inputs(ctx, [x for _, x, _ in CASES])]


@pytest.fixture(scope="module")
def host_statuses():
    import qp_wormhole
    return [tuple(s) for s in qp_wormhole.screen_inputs(None, [x for _, x, _ in CASES])]


@pytest.fixture(scope="module")
def circuit_verdicts(prover, circuit):
    """what the unchanged prove_inputs([x]) does with every case, computed once: ("proof", verify
    status) or ("error", code); and the code commit gives"""
    import qp_wormhole
    out, proofs = [], []
    for _, x, _ in CASES:
        try:
            proofs.append(prover.prove_inputs([x])[0])
            out.append(["proof", len(proofs) - 1, None])
        except qp_wormhole.QpError as e:
            try:
                circuit.commit(x)
                commit_code = 0
            except qp_wormhole.QpError as ce:
                commit_code = ce.code
            out.append(["error", e.code, commit_code])
    full, common = prover.verifier_data(), circuit.common_data()
    v = qp_wormhole.WormholeVerifier(circuit_data=(full[:len(full) - len(common)], common), device=0, max_batch=64)
    try:
        verdicts = v.verify_batch(proofs)
    finally:
        v.close()
    for o in out:
        if o[0] == "proof":
            o[1] = int(verdicts[o[1]])
    return out


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_device_equals_host_path_and_model(device_statuses, host_statuses, k):
    _, x, want = CASES[k]
    assert device_statuses[k] == host_statuses[k] == model(x) == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_lane_block_and_chunk_edges(ctx, n):
    """mixed-depth batches with a bad input in the first and in the last lane; 257 inputs are two
    blocks of k_screen_resolve and several of k_screen_nodes, 1025 cross the 1024-input upload chunk"""
    import qp_wormhole
    xs = mixed_batch(n)
    host = qp_wormhole.screen_inputs(None, xs)
    assert qp_wormhole.screen_inputs(ctx, xs) == host
    assert host[0].status >= NULLIFIER and host[-1].status >= NULLIFIER


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_screen_decides_what_the_circuit_decides(device_statuses, circuit_verdicts, k):
    """status >= 4: the unchanged prove_inputs([x]) raises QP_ERR_WITNESS; 1-3: the code commit gives;
    OK: a proof that WormholeVerifier accepts"""
    status = device_statuses[k][0]
    kind, a, b = circuit_verdicts[k]
    if status == OK:
        assert (kind, a) == ("proof", 0)
    elif status >= NULLIFIER:
        assert (kind, a) == ("error", 5)
    else:
        assert kind == "error" and a == b and a == 1


def _nine():
    """nine inputs, the bad ones at 0, 3 and 8"""
    good = [x for _, x, want in CASES if want[0] == OK][:6]
    bad = [x for _, x, want in CASES if want[0] in (1, 4, 6)]
    bad = [next(x for x in bad if model(x)[0] == s) for s in (6, 1, 4)]
    return [bad[0], good[0], good[1], bad[1], good[2], good[3], good[4], good[5], bad[2]], good


def test_skip_mode_at_the_batch_seam(prover):
    xs, good = _nine()
    proofs, statuses = prover.prove_inputs(xs, on_bad="skip")
    assert [tuple(s) for s in statuses] == [model(x) for x in xs]
    assert [p is None for p in proofs] == [i in (0, 3, 8) for i in range(9)]
    assert [p for p in proofs if p is not None] == prover.prove_inputs(good)


def test_skip_mode_all_good_and_all_bad(prover):
    xs, good = _nine()
    want = prover.prove_inputs(good[:5])
    proofs, statuses = prover.prove_inputs(good[:5], on_bad="skip")
    assert proofs == want and all(tuple(s) == (OK, 0) for s in statuses)
    bad = [xs[0], xs[3], xs[8]]
    proofs, statuses = prover.prove_inputs(bad, on_bad="skip")
    assert proofs == [None] * 3 and [tuple(s) for s in statuses] == [model(x) for x in bad]
    assert prover.prove_inputs(good[:1]) == want[:1]  # the prover is still usable
    assert prover.prove_inputs([], on_bad="skip") == ([], [])


def test_raise_mode_is_unchanged(prover):
    import qp_wormhole
    xs, _ = _nine()
    with pytest.raises(qp_wormhole.QpError) as e:
        prover.prove_inputs(xs[:3])
    assert e.value.code == 5 and "proof 0" in str(e.value)
    with pytest.raises(ValueError):
        prover.prove_inputs(xs, on_bad="drop")
