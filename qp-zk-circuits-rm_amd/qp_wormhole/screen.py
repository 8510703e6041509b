"""The screen of Wormhole circuit inputs (qp_wormhole_inputs_screen, include/qpgpu.h):
per input, what the circuit decides, as the first check that fails, without
building a witness.  With a Context the hashes run on the device; with None the
same rules run in the library's host C++."""
import ctypes
from collections import namedtuple

import numpy as np

from ._native import QpError, lib

# qp_input_status, in the order of the checks
INPUT_STATUS_TEXT = ("ok", "digest out of field range", "storage proof too long", "storage-proof node too large",
                     "wrong nullifier", "wrong unspendable account", "storage-proof node does not hash up",
                     "leaf hash not in the last node")

InputStatus = namedtuple("InputStatus", "status witness")


def input_status_text(status):
    """The library's one-line description of a status (qp_input_status_text)."""
    return lib().qp_input_status_text(int(status)).decode()


def screen_inputs(ctx, inputs):
    """[InputStatus(status, witness)] of a list of CircuitInputs: ctx a Context (device
    path, on its stream) or None (host path)."""
    n = len(inputs)
    if not n:
        return []
    structs = [x.to_c() for x in inputs]
    arr = (type(structs[0]) * n)(*structs)
    status, witness = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = lib().qp_wormhole_inputs_screen(ctx.h if ctx is not None else None, ctypes.cast(arr, ctypes.c_void_p), n,
                                         status.ctypes.data, witness.ctypes.data)
    if rc:
        if ctx is not None:
            ctx.check(rc, "qp_wormhole_inputs_screen")
        raise QpError(rc, "qp_wormhole_inputs_screen")
    return [InputStatus(int(s), int(w)) for s, w in zip(status, witness)]


def screen_times():
    """Times of this thread's last screen (ms): host checks and packing, then on the
    device path the upload, the node kernel and the resolve kernel."""
    ms = (ctypes.c_double * 4)()
    lib().qp_wormhole_inputs_screen_times(ms)
    return dict(zip(("pack", "upload", "nodes_kernel", "resolve_kernel"), ms))
