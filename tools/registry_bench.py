"""Times the voter registry on the device: the build of an N = 2^20 electorate
(wall time of VoterRegistry(ctx, keys) and the HIP-event times of its upload,
leaf and level kernels), `paths` for a 1024-voter batch, and, for comparison,
the host fallback's build at a size that takes about a second, scaled linearly
to N (labelled as scaled: it was not run at N).

The yardstick is not the new code: the same process proves one Wormhole batch
with kernel timing on and reports the prover's own leaf-hash and Merkle-level
rates (Prover.kernel_stats: the figures of bench.py --full's kernel table).

Writes one JSON object (default profiles/registry_bench.json) stamped with the
library hash (tools/libhash.py).  Needs an MI355X: without a device it fails.

  python tools/registry_bench.py [--log-n 20] [--batch 1024] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qp-zk-circuits-rm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 0xFFFFFFFF00000001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-log-n", type=int, default=16, help="size of the host-fallback build that is timed")
    ap.add_argument("--yardstick-batch", type=int, default=64, help="Wormhole proofs of the prover-rate run (0 = skip)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registry_bench.json"))
    args = ap.parse_args()

    import qp_wormhole
    from qp_wormhole import VoterRegistry
    from qp_wormhole._native import LIB_PATH
    from libhash import lib_sha16

    n = 1 << args.log_n
    rng = np.random.default_rng(1)
    keys = rng.integers(0, P, size=(n, 4), dtype=np.uint64)
    idx = rng.integers(0, n, args.batch)
    ctx = qp_wormhole.Context(0)

    VoterRegistry(ctx, keys).free()  # warm-up: code objects, allocator
    wall, dev = [], []
    reg = None
    for _ in range(args.reps):
        if reg is not None:
            reg.free()
        t0 = time.perf_counter()
        reg = VoterRegistry(ctx, keys)  # returns after the stream is synchronised
        wall.append(time.perf_counter() - t0)
        dev.append(reg.build_times())
    perms = 2 * n - 1  # n leaves + n - 1 nodes (a promoted node costs none)
    med = {k: statistics.median(d[k] for d in dev) for k in dev[0]}
    kernel_s = (med["leaves_ms"] + med["levels_ms"]) / 1e3

    reg.paths_raw(idx)  # warm-up
    pt = []
    for _ in range(max(args.reps, 20)):
        t0 = time.perf_counter()
        reg.paths_raw(idx)  # ends in a stream synchronise and the copies back
        pt.append(time.perf_counter() - t0)
    root = reg.root
    reg.free()

    hn = 1 << args.host_log_n
    t0 = time.perf_counter()
    host = VoterRegistry(None, keys[:hn])
    host_s = time.perf_counter() - t0
    # same tree convention: the device tree over the same keys has the same root
    small = VoterRegistry(ctx, keys[:hn])
    assert small.root == host.root, "device and host fallback disagree"
    small.free()

    yard = None
    if args.yardstick_batch:
        from qp_wormhole.synthetic import synthetic_inputs
        circ = qp_wormhole.Circuit.wormhole()
        prover = qp_wormhole.Prover(ctx, circ, args.yardstick_batch)
        arr = prover.inputs_array([synthetic_inputs(k, 3) for k in range(args.yardstick_batch)])
        prover.prove_inputs_array(arr, args.yardstick_batch)  # warm-up
        prover.set_timing(True)
        prover.kernel_stats(reset=True)
        for _ in range(3):
            prover.prove_inputs_array(arr, args.yardstick_batch)
        ks = prover.kernel_stats()
        yard = {"batch": args.yardstick_batch, "runs": 3,
                "leaf_hash_wires_perm_per_s": ks["leaf_hash_wires"]["units"] / ks["leaf_hash_wires"]["ms"] * 1e3,
                "merkle_wires_perm_per_s": ks["merkle_wires"]["units"] / ks["merkle_wires"]["ms"] * 1e3}
        prover.free()

    out = {
        "lib_sha16": lib_sha16(LIB_PATH),
        "voters": n, "levels": args.log_n + 1, "permutations": perms, "root": root,
        "build_wall_s": {"median": statistics.median(wall), "min": min(wall), "max": max(wall), "runs": len(wall),
                         "what": "VoterRegistry(ctx, keys): host check + key-major copy, upload, kernels, sync"},
        "build_device_ms": med,
        "build_kernels_perm_per_s": perms / kernel_s,
        "leaves_perm_per_s": n / (med["leaves_ms"] / 1e3),
        "levels_perm_per_s": (n - 1) / (med["levels_ms"] / 1e3),
        "build_wall_perm_per_s": perms / statistics.median(wall),
        "paths_batch": args.batch,
        "paths_wall_s": {"median": statistics.median(pt), "min": min(pt), "max": max(pt), "runs": len(pt),
                         "what": "paths_raw(1024 indices): index upload, k_registry_paths, copies back, sync"},
        "host_fallback": {"voters": hn, "build_s": host_s,
                          "build_s_scaled_to_voters": host_s * n / hn,
                          "note": "SCALED linearly from %d voters, not run at %d" % (hn, n)},
        "prover_yardstick": yard if yard else "not measured",
    }
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
