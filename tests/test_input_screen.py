"""The input screen's host path (qp_wormhole_inputs_screen with no context: the
rules of csrc/input_screen.h over the host Poseidon) against the Python model
on every case of wormhole_screen_model.py, and the model against the verdict
written down by hand for each case.  No device needed."""
import pytest

import qp_wormhole
from wormhole_screen_model import CASE_IDS, CASES, MAX_NODES, OK, mixed_batch, model


@pytest.fixture(scope="module")
def host_statuses():
    """the host path's verdicts on the whole table, one call"""
    return [tuple(s) for s in qp_wormhole.screen_inputs(None, [x for _, x, _ in CASES])]


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_model_gives_the_verdict_written_down(k):
    _, x, want = CASES[k]
    assert model(x) == want


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_host_path_equals_model(host_statuses, k):
    _, x, _ = CASES[k]
    assert host_statuses[k] == model(x)


@pytest.fixture(scope="module")
def circuit():
    return qp_wormhole.Circuit.wormhole()


@pytest.mark.parametrize("k", range(len(CASES)), ids=CASE_IDS)
def test_host_witness_generation_agrees(circuit, host_statuses, k):
    """the circuit itself on the host (commit: fill_targets + every generator): a witness for an OK
    input, QP_ERR_WITNESS for statuses 4-7, the argument error commit gives for 1-3"""
    _, x, _ = CASES[k]
    status = host_statuses[k][0]
    try:
        circuit.commit(x)
        code = 0
    except qp_wormhole.QpError as e:
        code = e.code
    assert code == (0 if status == OK else 5 if status >= 4 else 1)


def test_table_covers_what_it_must():
    """depths 0, 1, 2, 19, 20; node lengths 32, 61, 720, 752; every status; OK among them"""
    depths = {len(x.private.storage_proof.proof) for _, x, want in CASES if want[0] == OK}
    assert {0, 1, 2, 19, MAX_NODES} <= depths
    lens = {len(nd) for _, x, want in CASES if want[0] == OK for nd in x.private.storage_proof.proof}
    assert {32, 61, 720, 752} <= lens
    assert {want[0] for _, _, want in CASES} == set(range(8))
    starts = {i // 8 for _, x, want in CASES if want[0] == OK for i in x.private.storage_proof.indices}
    assert {0, 179} <= starts
    assert any(i % 8 for _, x, _ in CASES for i in x.private.storage_proof.indices)


def test_a_verdict_does_not_depend_on_the_neighbours(host_statuses):
    xs = mixed_batch(65)
    by_id = {id(x): host_statuses[k] for k, (_, x, _) in enumerate(CASES)}
    got = [tuple(s) for s in qp_wormhole.screen_inputs(None, xs)]
    assert got == [by_id[id(x)] for x in xs]
    assert got[0][0] >= 4 and got[-1][0] >= 4


def test_status_text():
    from qp_wormhole.screen import input_status_text
    assert len(qp_wormhole.INPUT_STATUS_TEXT) == 8
    texts = [input_status_text(s) for s in range(8)]
    assert len(set(texts)) == 8 and texts[0] == "ok" and "nullifier" in texts[4] and "leaf" in texts[7]
    assert input_status_text(8) == input_status_text(1 << 31) == "unknown input status"


def test_empty_list():
    assert qp_wormhole.screen_inputs(None, []) == []
