"""CPU-side checks of the commitment-registry part of the C ABI: include/qpgpu.h
declares the entry points with the arity the issue gives, libqpgpu.so exports
them, the ctypes table binds them, and the handle-less calls fail with a status
(no device needed)."""
import ctypes
import re

import numpy as np

import qp_wormhole
from qp_wormhole._native import HEADER

# name -> number of parameters in include/qpgpu.h
OPEN_SYMBOLS = {"qp_registry_new_commitments": 5, "qp_registry_append": 4, "qp_registry_replace": 4,
                "qp_registry_reserve": 2, "qp_registry_state": 3}


def test_symbols_declared_exported_and_bound():
    L = qp_wormhole.lib()
    declared = qp_wormhole.header_symbols()
    txt = open(HEADER).read()
    for s, arity in OPEN_SYMBOLS.items():
        assert s in declared, s
        f = getattr(L, s)  # exported
        assert f.argtypes is not None and len(f.argtypes) == arity, s  # bound in qp_wormhole._native
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % s, txt, re.M)
        assert m and len(m.group(1).split(",")) == arity, s


def test_null_handles_are_argument_errors():
    L = qp_wormhole.lib()
    h = ctypes.c_void_p()
    leaves = np.array([[1, 2, 3, 4]], np.uint64)
    assert L.qp_registry_new_commitments(None, leaves.ctypes.data, 1, 4, ctypes.byref(h)) == 1 and not h.value
    assert L.qp_registry_append(None, leaves.ctypes.data, 1, None) == 1
    assert L.qp_registry_replace(None, leaves.ctypes.data, leaves.ctypes.data, 1) == 1
    assert L.qp_registry_reserve(None, 8) == 1
    assert L.qp_registry_state(None, None, None) == 1


def test_python_surface():
    R = qp_wormhole.VoterRegistry
    for name in ("from_commitments", "commitment", "append", "replace", "reserve", "inputs_for", "capacity", "epoch",
                 "has_keys"):
        assert hasattr(R, name), name
