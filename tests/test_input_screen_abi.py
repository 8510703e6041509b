"""CPU-side checks of the input-screen part of the C ABI: include/qpgpu.h declares
the entry points, libqpgpu.so exports them, the ctypes table binds them with the
header's arity, the status enum is the order of the checks, and what the screen
refuses for the whole call (programming errors, not bad inputs) is QP_ERR_ARG."""
import ctypes
import os
import re

import numpy as np

import qp_wormhole
from wormhole_screen_model import CASES, NODE_TOO_LARGE, PROOF_TOO_LONG, model

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpgpu.h")

# name -> number of parameters in include/qpgpu.h
SYMBOLS = {"qp_wormhole_inputs_screen": 5, "qp_input_status_text": 1, "qp_prover_prove_wormhole_inputs_status": 8,
           "qp_wormhole_inputs_screen_times": 1}


def test_symbols_declared_exported_and_bound():
    L = qp_wormhole.lib()
    declared = qp_wormhole.header_symbols()
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for s, arity in SYMBOLS.items():
        assert s in declared, s
        f = getattr(L, s)
        assert f.argtypes is not None and len(f.argtypes) == arity, s
        m = re.search(r"^[\w ]+?\*?%s\s*\(([^)]*)\)\s*;" % s, txt, re.M)
        assert m and len(m.group(1).split(",")) == arity, s
    for name in ("screen_inputs", "InputStatus", "INPUT_STATUS_TEXT"):
        assert name in qp_wormhole.__all__ and hasattr(qp_wormhole, name)
    enum = re.search(r"typedef enum \{([^}]*)\} qp_input_status;", open(HEADER).read(), re.S).group(1)
    names = re.findall(r"QP_INPUT_(\w+) = (\d+)", enum)
    assert [int(v) for _, v in names] == list(range(8)) and len(qp_wormhole.INPUT_STATUS_TEXT) == 8
    assert [n for n, _ in names] == ["OK", "FIELD_RANGE", "PROOF_TOO_LONG", "NODE_TOO_LARGE", "NULLIFIER", "UNSPENDABLE",
                                     "STORAGE_NODE", "STORAGE_LEAF"]


def _screen(structs, status=True, witness=True):
    n = len(structs)
    arr = (type(structs[0]) * n)(*structs)
    st, wi = np.full(n, 77, np.uint32), np.full(n, 77, np.uint32)
    rc = qp_wormhole.lib().qp_wormhole_inputs_screen(None, ctypes.cast(arr, ctypes.c_void_p), n,
                                                     st.ctypes.data if status else None,
                                                     wi.ctypes.data if witness else None)
    return rc, st, wi


def _case(name):
    return next(x for n, x, _ in CASES if n == name)


def test_null_arrays_are_argument_errors():
    L = qp_wormhole.lib()
    good = _case("depth5_mixed_lengths").to_c()
    assert L.qp_wormhole_inputs_screen(None, None, 1, None, None) == 1
    assert _screen([good], status=False)[0] == 1
    assert _screen([good], witness=False)[0] == 1
    assert L.qp_wormhole_inputs_screen(None, None, 0, None, None) == 0  # nothing to screen
    assert L.qp_prover_prove_wormhole_inputs_status(None, None, 0, None, 0, None, None, None) == 1
    assert L.qp_wormhole_inputs_screen_times(None) == 1


def test_null_storage_proof_pointers_refuse_the_whole_call():
    """a null array or node where num_nodes announces data is a programming error: QP_ERR_ARG, and no
    verdict is written for any input of the call, the good ones included"""
    for field in ("nodes", "node_lens", "indices"):
        good, broken = _case("depth2_len61_len752_felt179_hexoff").to_c(), _case("depth5_mixed_lengths").to_c()
        setattr(broken, field, None)
        rc, st, wi = _screen([good, broken])
        assert rc == 1 and (st == 77).all() and (wi == 77).all(), field
    # also where the count alone would be refused as a bad input
    broken = _case("proof_21_nodes").to_c()
    broken.nodes = None
    assert _screen([broken])[0] == 1
    # a null node with a length
    broken = _case("depth5_mixed_lengths").to_c()
    broken.nodes[3] = None
    assert _screen([broken])[0] == 1
    # num_nodes == 0 reads none of the three
    empty = _case("depth0").to_c()
    assert not empty.nodes and _screen([empty])[0] == 0


def test_a_null_node_of_length_zero_is_an_empty_node():
    x = _case("depth5_mixed_lengths")
    s = x.to_c()
    s.nodes[4] = None
    s.node_lens[4] = 0
    rc, st, wi = _screen([s])
    assert rc == 0 and (int(st[0]), int(wi[0])) == (6, 4)  # STORAGE_NODE: the empty node hashes to something else


def test_bad_inputs_are_verdicts_not_errors():
    for name, want in (("proof_21_nodes", PROOF_TOO_LONG), ("node_753_bytes", NODE_TOO_LARGE)):
        rc, st, wi = _screen([_case(name).to_c()])
        assert rc == 0 and (int(st[0]), int(wi[0])) == model(_case(name)) and st[0] == want


def test_screen_times_are_the_last_call_of_the_thread():
    from qp_wormhole.screen import screen_times
    qp_wormhole.screen_inputs(None, [_case("depth19")])
    t = screen_times()
    assert t["pack"] == 0 and t["upload"] == 0 and t["nodes_kernel"] == 0 and t["resolve_kernel"] == 0
