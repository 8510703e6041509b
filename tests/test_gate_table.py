"""The library's one gate table (csrc/gates.h) against what the code before
it computed: tests/golden/gate_table.json was written by the commit that still
had a kind numbering per component, a shape switch in the qp_quotient seam and
another in the verifier.

  census       Circuit.census() of the Wormhole leaf circuit and of a level-1
               aggregation circuit: qp_circuit_census' rows[] keep the ABI's
               order, whatever the kind enum's is.
  shapes       per kind, at the builder's parameters and at the boundary ones,
               the wires / gate constants / constraints the seam validated
               with and the verifier validated with, and whether each took
               the gate in a circuit of 135 wires, 2 gate constants and 123
               gate constraints.  gates.h is walked by a stand-alone program
               (tests/gate_table_walk.cpp, also the host-sanitizer program).
  verifier_new the verifier's constructor on the aggregation circuit's common
               data with one gate's parameters replaced: status and message.
"""
import ctypes
import json
import os
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
with open(os.path.join(HERE, "golden", "gate_table.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def agg_circuit():
    from qp_wormhole import Circuit
    from test_oracle_golden import current_common_bytes
    return Circuit.aggregation(current_common_bytes(), 2)


def test_census_keeps_the_abi_order(agg_circuit):
    from qp_wormhole import Circuit
    for name, circ in (("wormhole", Circuit.wormhole()), ("aggregation", agg_circuit)):
        gens, rows = circ.census()
        assert gens == GOLDEN["census"][name]["gens"], name
        assert rows == GOLDEN["census"][name]["rows"], name


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    """gate_shape / serial_id / kind_from_serial of every case, from gates.h itself."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/bin/hipcc")
                if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("gate_table") / "walk")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "gate_table_walk.cpp"),
                           "-o", exe])
    args = [str(x) for c in GOLDEN["shapes"] for x in [c["kind_id"]] + c["params"]]
    return json.loads(subprocess.check_output([exe] + args))


def test_shapes_equal_the_seams_and_the_verifiers(walked):
    assert len(walked) == len(GOLDEN["shapes"]) >= 14
    assert {c["kind_id"] for c in GOLDEN["shapes"]} == set(range(14))
    ctx = GOLDEN["context"]
    for want, got in zip(GOLDEN["shapes"], walked):
        tag = (want["kind"], want["params"])
        assert got["serial_id"] == want["serial_id"] and got["kind_from_serial"] == want["kind_id"], tag
        shape = {k: got[k] for k in ("wires", "consts", "constraints")}
        fits = (got["ok"] and got["wires"] <= ctx["num_wires"] and got["consts"] <= ctx["gate_constants"] and
                got["constraints"] <= ctx["num_gate_constraints"])
        seam, ver = want["seam"], want["verifier"]
        # the seam: gate_shape's bounds, and at least one coefficient for the Reducing gates (its call site)
        no_coeffs = want["kind"] in ("reducing", "reducing_extension") and want["params"][0] < 1
        assert (got["ok"] and not no_coeffs) == seam["ok"], tag
        if seam["ok"]:
            assert shape == {k: seam[k] for k in shape}, tag
        assert (fits and not no_coeffs) == seam["accept"], tag
        # the verifier: the same numbers wherever it computed any
        if ver["shape"] is not None and got["ok"]:
            assert shape == ver["shape"], tag


def test_rejected_boundaries_are_recorded():
    """What the seam and the verifier each did with the boundary parameters
    (the verifier's side: its constructor's status, checked against the library
    in test_verifier_constructor_takes_and_refuses_as_before)."""
    seam = {(c["kind"], c["case"]): c["seam"]["accept"] for c in GOLDEN["shapes"]}
    ver = {(c["kind"], c["case"]): c["rc"] == 0 for c in GOLDEN["verifier_new"]}
    for key in (("random_access", "bits 0"), ("random_access", "bits 7"), ("coset_interpolation", "degree 1")):
        assert (seam[key], ver[key]) == (False, False), key
    # zero Reducing coefficients: the seam refuses, the verifier takes them
    for key in (("reducing", "0 coefficients"), ("reducing_extension", "0 coefficients")):
        assert (seam[key], ver[key]) == (False, True), key


def patched_common(cb, tag, old, new_tag, new):
    """cb with the gate of serializer tag `tag` and parameters `old` replaced by (new_tag, new)."""
    pat = struct.pack("<I", tag) + struct.pack("<%dQ" % len(old), *old)
    assert cb.count(pat) == 1
    return cb.replace(pat, struct.pack("<I", new_tag) + struct.pack("<%dQ" % len(new), *new))


def test_verifier_constructor_takes_and_refuses_as_before(agg_circuit):
    import verifier_cases as vc
    from qp_wormhole import lib
    vo, cb = vc.current_vd()[0], agg_circuit.common_data()
    for case in GOLDEN["verifier_new"]:
        data = cb
        if case["tag"] is not None:
            data = patched_common(cb, case["tag"], case["old"], case["new_tag"], case["new"])
        h = ctypes.c_void_p()
        rc = lib().qp_verifier_new(None, vo, len(vo), data, len(data), 4, ctypes.byref(h))
        msg = lib().qp_verifier_last_error(h).decode() if h else ""
        lib().qp_verifier_free(h)
        assert (rc, msg) == (case["rc"], case["message"]), case
