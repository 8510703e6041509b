"""The field-arithmetic edge values the GPU tests share (test infrastructure):
the operands around 0, 2^31, 2^32, 2^63, p = 2^64 - 2^32 + 1 and 2^64 at which
the device's carry chains wrap, borrow or canonicalise."""
import numpy as np

P = 0xFFFFFFFF00000001

EDGES = [0, 1, 2, 2**31, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**33 - 1, 2**63 - 1, 2**63, 2**63 + 1,
         P - 2**32 - 1, P - 2**32, P - 2**32 + 1, P - 2, P - 1, P, P + 1, P + 2**32 - 2, 2**64 - 2**32 - 1,
         2**64 - 2**32, 2**64 - 2**32 + 1, 2**64 - 2, 2**64 - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF,
         0x8000000080000000]
# the field elements among them, duplicates dropped, order kept
CANON_EDGES = list(dict.fromkeys(v for v in EDGES if v < P))


def edge_cycle(n, start=0):
    """n canonical edge values, cycling through the list from `start`."""
    k = len(CANON_EDGES)
    return np.array([CANON_EDGES[(start + i) % k] for i in range(n)], dtype=np.uint64)


def constant_columns(ncols, n, start=0):
    """[ncols][n]: column j constant at canonical edge value (start + j) mod k.
    A constant column has a constant LDE, so every value a kernel reads from
    its extension is that edge value."""
    return np.repeat(edge_cycle(ncols, start)[:, None], n, axis=1)


def bitrev_perm(bits):
    """rev[i] = i with its low `bits` bits reversed."""
    i = np.arange(1 << bits, dtype=np.int64)
    r = np.zeros_like(i)
    for k in range(bits):
        r |= ((i >> k) & 1) << (bits - 1 - k)
    return r
