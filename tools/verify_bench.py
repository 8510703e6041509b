"""Verifier throughput on the GPU: a batch of Wormhole proofs from this
backend's prover through WormholeVerifier.verify_batch (device), a single-proof
verify, and the reference's bench shape (verifier/benches/verifier.rs:
new_from_files once, then verify of bench-data's proof.bin); beside them, in the
same run, the library's own host path and the checker (ora_verify on 16
threads).  Host clock around calls that end synchronised.

  python tools/verify_bench.py [--batch 256] [--window 1.0] [--out profiles/verifier_bench.json] [--kernels-only]

--kernels-only: warm up, then a few verify_batch calls and nothing else (the
program to put after `rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "qp-zk-circuits-rm_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def timed(fn, window, min_reps=3):
    """(seconds per call, reps) over at least `window` seconds."""
    reps, t0 = 0, time.perf_counter()
    while True:
        fn()
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= window and reps >= min_reps:
            return dt / reps, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_bench.json"))
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()

    import qp_wormhole
    from libhash import lib_sha16
    from oracle_lib import GOLDEN, golden, lib as olib
    from qp_wormhole.synthetic import synthetic_inputs

    B = a.batch
    ctx = qp_wormhole.Context(0)
    circ = qp_wormhole.Circuit.wormhole()
    prover = qp_wormhole.Prover(ctx, circ, max_batch=min(B, 64))
    proofs = prover.prove_witnesses([circ.commit(synthetic_inputs(k, k % 3)) for k in range(B)])
    vd, cb = prover.verifier_data(), circ.common_data()
    vo = vd[:len(vd) - len(cb)]
    prover.free()

    dev = qp_wormhole.WormholeVerifier.new_from_bytes(vo, cb, device=0, max_batch=B)
    assert dev.verify_batch(proofs) == [0] * B  # warm-up, and the batch is what it should be
    if a.kernels_only:
        for _ in range(5):
            dev.verify_batch(proofs)
        return
    res = {"command": "python tools/verify_bench.py --batch %d --window %g" % (B, a.window), "lib_sha16": lib_sha16(),
           "batch": B, "proof_bytes": len(proofs[0]), "host_threads": min(os.cpu_count() or 4, 16)}
    s, reps = timed(lambda: dev.verify_batch(proofs), a.window)
    res["gpu_batch"] = {"proofs_per_s": B / s, "ms_per_batch": s * 1e3, "reps": reps}
    s, reps = timed(lambda: dev.verify(proofs[0]), a.window)
    res["gpu_single"] = {"ms_per_proof": s * 1e3, "reps": reps}

    host = qp_wormhole.WormholeVerifier.new_from_bytes(vo, cb, device=None, max_batch=B)
    assert host.verify_batch(proofs[:16]) == [0] * 16
    s, reps = timed(lambda: host.verify_batch(proofs), a.window)
    res["host_path_batch"] = {"proofs_per_s": B / s, "ms_per_batch": s * 1e3, "reps": reps}
    s, reps = timed(lambda: host.verify(proofs[0]), a.window)
    res["host_path_single"] = {"ms_per_proof": s * 1e3, "reps": reps}

    L = olib()
    pool = ThreadPoolExecutor(16)  # ctypes releases the GIL in ora_verify

    def oracle_batch():
        assert not any(pool.map(lambda p: L.ora_verify(vd, len(vd), p, len(p)), proofs))
    s, reps = timed(oracle_batch, a.window)
    res["oracle_16_threads"] = {"proofs_per_s": B / s, "ms_per_batch": s * 1e3, "reps": reps}

    # the reference's bench shape
    t0 = time.perf_counter()
    ref = qp_wormhole.WormholeVerifier.new_from_files(os.path.join(GOLDEN, "verifier.bin"),
                                                      os.path.join(GOLDEN, "common.bin"), max_batch=1)
    t_new = time.perf_counter() - t0
    pf = golden("proof.bin")
    ref.verify(pf)
    s, reps = timed(lambda: ref.verify(pf), a.window)
    res["reference_bench_shape"] = {"new_from_files_ms": t_new * 1e3, "verify_ms": s * 1e3, "reps": reps}
    ref_host = qp_wormhole.WormholeVerifier.new_from_files(os.path.join(GOLDEN, "verifier.bin"),
                                                           os.path.join(GOLDEN, "common.bin"), device=None, max_batch=1)
    s, reps = timed(lambda: ref_host.verify(pf), a.window)
    res["reference_bench_shape"]["host_path_verify_ms"] = s * 1e3
    vb = golden("verifier.bin")
    s, reps = timed(lambda: L.ora_verify(vb, len(vb), pf, len(pf)), a.window)
    res["reference_bench_shape"]["oracle_verify_ms"] = s * 1e3

    for v in (dev, host, ref, ref_host):
        v.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
