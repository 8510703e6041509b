"""CPU-side checks of the voter-registry part of the C ABI: include/qpgpu.h
declares the entry points, libqpgpu.so exports them, the ctypes table binds
them, and the handle-less calls fail with a status (no device needed)."""
import ctypes

import numpy as np

import qp_wormhole

REGISTRY_SYMBOLS = ["qp_registry_new", "qp_registry_root", "qp_registry_size", "qp_registry_free",
                    "qp_registry_paths", "qp_prover_prove_voters"]


def test_registry_symbols_declared_and_exported():
    L = qp_wormhole.lib()
    declared = qp_wormhole.header_symbols()
    for s in REGISTRY_SYMBOLS + ["qp_registry_level", "qp_registry_build_times"]:
        assert s in declared, s
        f = getattr(L, s)
        assert f.argtypes is not None, s  # bound in qp_wormhole._native


def test_null_handles_are_argument_errors():
    L = qp_wormhole.lib()
    h = ctypes.c_void_p()
    keys = np.array([[1, 2, 3, 4]], np.uint64)
    assert L.qp_registry_new(None, keys, 1, ctypes.byref(h)) == 1 and not h.value
    assert L.qp_registry_root(None, np.zeros(4, np.uint64)) == 1
    assert L.qp_registry_size(None, None, None) == 1
    assert L.qp_registry_paths(None, keys.ravel(), 1, np.zeros(128, np.uint64), np.zeros(1, np.uint32),
                               np.zeros(1, np.uint32)) == 1
    assert L.qp_registry_level(None, 0, None, None) == 1
    assert L.qp_prover_prove_voters(None, None, keys.ravel(), None, 1, None, 0, None) == 1
    L.qp_registry_free(None)


def test_exported_from_the_package():
    assert "VoterRegistry" in qp_wormhole.__all__
    assert qp_wormhole.VoterRegistry.__module__ == "qp_wormhole.registry"
