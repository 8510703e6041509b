"""WormholeVerifier: host-side mirror of the reference's qp-wormhole-verifier
(wormhole/verifier/src/lib.rs:81-159: new, new_from_bytes, new_from_files,
verify) over the native batch verifier (include/qpgpu.h qp_verifier_*).

The per-proof work (parse, transcript, vanishing identity, PoW) runs on a host
pool, the query rounds of the whole batch as HIP kernels on the device;
device=None runs the query rounds on the host too and needs no GPU.
verify_batch is this backend's addition.
"""
import ctypes
import struct

import numpy as np

from ._native import Context, QpError, lib

# qp_verify_status, worded as plonky2's verify / verify_fri_proof checks
STATUS_TEXT = ("ok", "public-input count mismatch", "zeta in subgroup", "vanishing/quotient identity",
               "pow response", "initial merkle path", "fri layer consistency", "fri layer merkle path",
               "final polynomial", "malformed proof")


def merkle_verify(ctx, leaves, idx, siblings, cap):
    """verify_merkle_proof_to_cap for n (leaf, index, siblings) triples against one cap, on the
    device: leaves [n][width], idx [n], siblings [n][nsib][4], cap [2^h][4] -> bool array [n]."""
    leaves = np.ascontiguousarray(leaves, dtype=np.uint64)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    cap = np.ascontiguousarray(cap, dtype=np.uint64).reshape(-1, 4)
    n, width = leaves.shape
    sib = np.ascontiguousarray(siblings, dtype=np.uint64)
    nsib = sib.size // (4 * n) if n else 0
    if sib.size != n * nsib * 4:
        raise ValueError("siblings must be [n][nsib][4]")
    if not sib.size:
        sib = np.zeros(4, np.uint64)
    cap_height = cap.shape[0].bit_length() - 1
    if cap.shape[0] != 1 << cap_height or idx.shape != (n,):
        raise ValueError("cap must hold 2^h digests and idx one entry per leaf")
    ok = np.zeros(max(n, 1), np.uint8)
    ctx.check(lib().qp_merkle_verify(ctx.h, leaves, width, idx, sib, nsib, cap, cap_height, n, ok), "qp_merkle_verify")
    return ok[:n].astype(bool)


def _split_verifier_only(verifier_bytes):
    """The VerifierOnlyCircuitData prefix of verifier_bytes (from_bytes reads cap
    height, cap and digest and leaves what follows: the reference's
    bench-data/verifier.bin carries the common data after it)."""
    b = bytes(verifier_bytes)
    if len(b) < 8:
        return None
    h = struct.unpack_from("<Q", b)[0]
    if h > 16:
        return None
    need = 8 + (32 << h) + 32
    return b[:need] if len(b) >= need else None


class WormholeVerifier:
    def __init__(self, config="standard_recursion_config", circuit_data=None, device=0, max_batch=256):
        """WormholeVerifier::new: circuit_data = (verifier_only_bytes, common_bytes), or None for
        the data of the built Wormhole circuit of `config` (as generate_circuit_binaries
        writes it; building it needs the device)."""
        if circuit_data is None:
            from .prover import CONFIGS, _shared, _verifier_only
            if config not in CONFIGS:
                raise ValueError(f"unknown circuit config {config!r}")
            ctx, circ, prover, lock = _shared(config, 0 if device is None else device)
            with lock:
                circuit_data = (_verifier_only(circ, prover), circ.common_data())
        verifier_only, common = circuit_data
        self._init(bytes(verifier_only), bytes(common), device, max_batch)

    def _init(self, verifier_only, common, device, max_batch):
        self.verifier_only, self.common = verifier_only, common
        self.device, self.max_batch = device, int(max_batch)
        self.ctx = None if device is None else Context(device)
        L = lib()
        h = ctypes.c_void_p()
        rc = L.qp_verifier_new(None if self.ctx is None else self.ctx.h, verifier_only, len(verifier_only), common,
                               len(common), self.max_batch, ctypes.byref(h))
        if rc:
            msg = L.qp_verifier_last_error(h).decode() if h else "qp_verifier_new"
            if h:
                L.qp_verifier_free(h)
            self.h = None
            raise QpError(rc, msg)
        self.h = h

    @classmethod
    def new_from_bytes(cls, verifier_bytes, common_bytes, device=0, max_batch=256):
        """WormholeVerifier::new_from_bytes (lib.rs:98-114), with its error messages."""
        vo = _split_verifier_only(verifier_bytes)
        if vo is None:
            raise ValueError("Failed to deserialize verifier data from bytes")
        self = cls.__new__(cls)
        try:
            self._init(vo, bytes(common_bytes), device, max_batch)
        except QpError as e:
            if e.code != 6:
                raise
            what = "verifier data" if "verifier data:" in str(e) else "common circuit data"
            raise ValueError(f"Failed to deserialize {what} from bytes") from e
        return self

    @classmethod
    def new_from_files(cls, verifier_data_path, common_data_path, device=0, max_batch=256):
        """WormholeVerifier::new_from_files (lib.rs:118-148)."""
        with open(verifier_data_path, "rb") as f:
            verifier_bytes = f.read()
        vo = _split_verifier_only(verifier_bytes)
        if vo is None:
            raise ValueError(f"Failed to deserialize verifier data from {str(verifier_data_path)!r}: "
                             "buffer too short")
        with open(common_data_path, "rb") as f:
            common = f.read()
        self = cls.__new__(cls)
        try:
            self._init(vo, common, device, max_batch)
        except QpError as e:
            if e.code != 6:
                raise
            what, path = (("verifier data", verifier_data_path) if "verifier data:" in str(e)
                          else ("common circuit data", common_data_path))
            raise ValueError(f"Failed to deserialize {what} from {str(path)!r}: {e}") from e
        return self

    def last_error(self):
        return lib().qp_verifier_last_error(self.h).decode()

    def set_host_threads(self, nthreads):
        rc = lib().qp_verifier_set_host_threads(self.h, int(nthreads))
        if rc:
            raise QpError(rc, "qp_verifier_set_host_threads")

    def verify_batch(self, proofs):
        """qp_verify_status of each proof (bytes or ProofWithPublicInputs); 0 = verified."""
        datas = [p if isinstance(p, (bytes, bytearray, memoryview)) else p.to_bytes() for p in proofs]
        datas = [bytes(d) for d in datas]
        n = len(datas)
        if self.h is None:
            raise QpError(4, "verifier is closed")
        ptrs = (ctypes.c_char_p * max(n, 1))(*datas)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in datas])
        status = (ctypes.c_uint32 * max(n, 1))()
        rc = lib().qp_verifier_verify(self.h, ptrs, lens, n, status)
        if rc:
            raise QpError(rc, f"qp_verifier_verify: {self.last_error()}")
        return [int(status[i]) for i in range(n)]

    def verify(self, proof):
        """WormholeVerifier::verify (lib.rs:155-159)."""
        st = self.verify_batch([proof])[0]
        if st:
            raise ValueError(f"proof verification failed: {STATUS_TEXT[st] if st < len(STATUS_TEXT) else st}")

    def close(self):
        if getattr(self, "h", None):
            lib().qp_verifier_free(self.h)
            self.h = None
        if getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
