"""Times the voter registry on the device: the build of an N = 2^20 electorate
(wall time of VoterRegistry(ctx, keys) and the HIP-event times of its upload,
leaf and level kernels), `paths` for a 1024-voter batch, and, for comparison,
the host fallback's build at a size that takes about a second, scaled linearly
to N (labelled as scaled: it was not run at N).

The commitment registry (from_commitments / append / replace / reserve) is
timed at the same N: every update beside a full from_commitments rebuild of the
tree it leaves, in the same process, wall and HIP events
(qp_registry_build_times: upload, levels), and the row form of the narrow
dirty ranges against the one-lane form (QPGPU_PATHS registry_row) per append
size, with intermediate bounds for the widest append.

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


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def open_registry_records(ctx, VoterRegistry, n, reps, rng):
    """from_commitments, append, replace and reserve at n voters, each beside a full
    rebuild of the resulting tree; the row / one-lane A/B of the update kernels"""
    appends = [1, 1024, 1 << 16]
    leaves = rng.integers(0, P, size=(n + max(appends), 4), dtype=np.uint64)

    def build(count, capacity=None):
        t0 = time.perf_counter()
        reg = VoterRegistry.from_commitments(ctx, leaves[:count], capacity=capacity)
        wall = time.perf_counter() - t0
        return reg, wall, reg.build_times()

    def rebuilds(count):
        w, up, lv = [], [], []
        for _ in range(reps):
            reg, wall, ms = build(count)
            reg.free()
            w.append(wall), up.append(ms["upload_ms"]), lv.append(ms["levels_ms"])
        return {"voters": count, "wall_s": _stats(w), "upload_ms": _stats(up), "levels_ms": _stats(lv)}

    def append_run(k, hook):
        """reps appends of k onto fresh n-voter registries under QPGPU_PATHS=hook (None: default)"""
        w, up, lv = [], [], []
        for _ in range(reps):
            reg = build(n, 2 * n)[0]  # built under the default paths
            if hook is not None:
                os.environ["QPGPU_PATHS"] = hook
            try:
                t0 = time.perf_counter()
                reg.append(leaves[n:n + k], reserve=False)
                w.append(time.perf_counter() - t0)
            finally:
                os.environ.pop("QPGPU_PATHS", None)
            ms = reg.build_times()
            root = reg.root
            reg.free()
            up.append(ms["upload_ms"]), lv.append(ms["levels_ms"])
        return {"wall_s": _stats(w), "upload_ms": _stats(up), "levels_ms": _stats(lv)}, root

    build(n)[0].free()  # warm-up
    out = {"from_commitments": rebuilds(n), "append": [], "row_ab": []}
    for k in appends:
        rec, root = append_run(k, None)
        full = rebuilds(n + k)
        check = build(n + k)[0]
        assert check.root == root, "append and rebuild disagree"
        check.free()
        rec.update({"k": k, "onto": n, "full_rebuild": full,
                    "wall_ratio_to_rebuild": rec["wall_s"]["median"] / full["wall_s"]["median"],
                    "levels_ratio_to_rebuild": rec["levels_ms"]["median"] / full["levels_ms"]["median"]})
        out["append"].append(rec)
    # the A/B: the levels' HIP-event time per append size with the row form always, never, and bounded
    for k in [1, 16, 256, 1024, 4096, 1 << 14, 1 << 16]:
        row = {"k": k}
        for name, hook in (("row_always", "registry_row=2147483648"), ("one_lane", "registry_row=0"),
                           ("row_below_256", "registry_row=256"), ("row_below_4096", "registry_row=4096"),
                           ("row_below_32768", "registry_row=32768")):
            row[name + "_levels_ms"] = append_run(k, hook)[0]["levels_ms"]["median"]
        out["row_ab"].append(row)
    # replace of 1024 scattered voters, repeated on one registry
    reg = build(n)[0]
    idx = rng.choice(n, 1024, replace=False)
    new = rng.integers(0, P, size=(1024, 4), dtype=np.uint64)
    reg.replace(idx, new)  # warm-up
    rep = {}
    for name, hook in (("default", None), ("row_always", "registry_row=2147483648"), ("one_lane", "registry_row=0")):
        if hook:
            os.environ["QPGPU_PATHS"] = hook
        w, lv = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            reg.replace(idx, new)
            w.append(time.perf_counter() - t0)
            lv.append(reg.build_times()["levels_ms"])
        os.environ.pop("QPGPU_PATHS", None)
        rep[name] = {"wall_s": _stats(w), "levels_ms": _stats(lv)}
    reg.free()
    rep.update({"k": 1024, "voters": n, "full_rebuild": "from_commitments above",
                "wall_ratio_to_rebuild": rep["default"]["wall_s"]["median"]
                / out["from_commitments"]["wall_s"]["median"]})
    out["replace"] = rep
    # reserve n -> 2 n: a device-to-device move of every level
    w = []
    for _ in range(reps):
        reg = build(n, n)[0]
        t0 = time.perf_counter()
        reg.reserve(2 * n)
        w.append(time.perf_counter() - t0)
        reg.free()
    out["reserve"] = {"from": n, "to": 2 * n, "wall_s": _stats(w)}
    return out


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

    opened = open_registry_records(ctx, VoterRegistry, n, args.reps, rng)

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
                         "what": "paths_raw(1024 indices): index upload, k_acc_paths, copies back, sync"},
        "host_fallback": {"voters": hn, "build_s": host_s,
                          "build_s_scaled_to_voters": host_s * n / hn,
                          "note": "SCALED linearly from %d voters, not run at %d" % (hn, n)},
        "prover_yardstick": yard if yard else "not measured",
        "commitment_registry": opened,
    }
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
