"""CPU-side checks of the partial-products, opening-set and FRI-polynomial
seams: the header declares them, the library exports them, and the Python
wrappers reject wrongly shaped arrays before anything reaches the library."""
import numpy as np
import pytest

import qp_wormhole
from qp_wormhole import _native

NEW = ["qp_perm_new", "qp_perm_free", "qp_partial_products_and_zs", "qp_opening_set", "qp_batch_eval_ext",
       "qp_fri_initial_poly"]


def test_new_seams_declared_and_exported():
    syms = qp_wormhole.header_symbols()
    L = qp_wormhole.lib()
    for s in NEW:
        assert s in syms, s
        assert hasattr(L, s), s
        assert getattr(L, s).argtypes is not None, s  # bound with a signature
    for name in ("PermutationData", "opening_set", "fri_initial_poly"):
        assert name in qp_wormhole.__all__ and hasattr(qp_wormhole, name)
    assert hasattr(qp_wormhole.PolynomialBatch, "eval_ext")


class _NoLibrary:
    """stands where a Context or a handle would: touching it means the wrapper went past its checks"""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached the library ({name})")


def _perm(num_routed=4, n=64):
    p = object.__new__(_native.PermutationData)
    p.ctx, p.h, p.num_routed, p.n = _NoLibrary(), None, num_routed, n
    return p


def test_permutation_data_rejects_bad_shapes():
    z = np.zeros
    for sigmas, k in [(z(64, np.uint64), z(1, np.uint64)),          # not a matrix
                      (z((4, 48), np.uint64), z(4, np.uint64)),     # rows not a power of two
                      (z((4, 64), np.uint64), z(3, np.uint64)),     # one k_i per column
                      (z((4, 64), np.uint64), z((4, 1), np.uint64))]:
        with pytest.raises(ValueError):
            _native.PermutationData(_NoLibrary(), sigmas, k)
    p = _perm()
    for wires, qdf, betas, gammas in [(z((4, 32), np.uint64), 8, [1, 2], [3, 4]),   # another degree
                                      (z((3, 64), np.uint64), 8, [1, 2], [3, 4]),   # routed columns missing
                                      (z(256, np.uint64), 8, [1, 2], [3, 4]),
                                      (z((4, 64), np.uint64), 8, [1, 2], [3]),      # challenges unpaired
                                      (z((4, 64), np.uint64), 8, [], []),
                                      (z((4, 64), np.uint64), 0, [1, 2], [3, 4])]:
        with pytest.raises(ValueError):
            p.partial_products_and_zs(wires, qdf, betas, gammas)


def test_eval_ext_rejects_bad_points_and_windows():
    b = _native.PolynomialBatch(_NoLibrary(), None, 4, 0, 3, 3, 0, None)
    for pts, first, npolys in [([1, 2], 0, None),            # one point must still be [1][2]
                               ([[1, 2, 3]], 0, None),
                               (np.zeros((0, 2), np.uint64), 0, None),
                               ([[1, 2]], 3, 2),             # window past the batch
                               ([[1, 2]], 4, None),          # empty window
                               ([[1, 2]], -1, 2),
                               ([[1, 2]], 0, 0)]:
        with pytest.raises(ValueError):
            b.eval_ext(pts, first, npolys)
    b.h = None


def test_opening_seams_reject_bad_points():
    b = _native.PolynomialBatch(_NoLibrary(), None, 4, 0, 6, 3, 0, None)
    with pytest.raises(ValueError):
        _native.opening_set(_NoLibrary(), b, b, b, b, 2, [1, 2, 3])
    with pytest.raises(ValueError):
        _native.fri_initial_poly(_NoLibrary(), b, b, b, b, 2, [1], [1, 2])
    b.h = None
