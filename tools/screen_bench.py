"""Times the Wormhole input screen and the prove call built on it, on batches of
256 inputs with the benchmark's depth mix (synthetic_inputs(k), depth seeded in
0..20):

  screen      qp_wormhole.screen_inputs of 256 inputs on the device (wall, and the
              call's own figures: host packing, upload, the two kernels'
              HIP-event times) beside the host path of the same library; the
              verdicts of the two paths are compared.  The ctypes structs are
              made beforehand for the `abi` rows, which time the C call alone.
  prove       Prover.prove_inputs(on_bad="skip") on an all-good batch of 256
              beside plain prove_inputs, same prover, same process, runs
              alternating; the proofs are compared.
  three_bad   256 inputs of which 3 do not satisfy the circuit: what finding
              them costs today (prove_inputs, drop the input the error names,
              again: four passes) beside one on_bad="skip" call.

Medians of --reps runs after one warm-up run.  Reported, not gated.  Writes one
JSON object (default profiles/screen_bench.json) stamped with the library hash
(tools/libhash.py).  Needs an MI355X: without a device it fails.

  python tools/screen_bench.py [--n 256] [--reps 5] [--out FILE]
"""
import argparse
import copy
import ctypes
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qp-zk-circuits-rm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def _ms(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def bench_screen(qp, ctx, xs, reps):
    from qp_wormhole.screen import screen_times
    n = len(xs)
    structs = [x.to_c() for x in xs]
    arr = (type(structs[0]) * n)(*structs)
    st, wi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    L = qp.lib()

    def abi(h):
        rc = L.qp_wormhole_inputs_screen(h, ctypes.cast(arr, ctypes.c_void_p), n, st.ctypes.data, wi.ctypes.data)
        assert rc == 0, rc
        return st.copy(), wi.copy()

    dev = abi(ctx.h)  # warm-up: the kernels' code objects load
    host = abi(None)
    assert (dev[0] == host[0]).all() and (dev[1] == host[1]).all()
    rows = {"device_abi": [], "host_abi": [], "device_python": [], "pack": [], "upload": [], "nodes_kernel": [],
            "resolve_kernel": []}
    for _ in range(reps):
        rows["device_abi"].append(_ms(lambda: abi(ctx.h))[0])
        for k, v in screen_times().items():
            rows[k].append(v)
        rows["host_abi"].append(_ms(lambda: abi(None))[0])
        rows["device_python"].append(_ms(lambda: qp.screen_inputs(ctx, xs))[0])
    nodes = sum(len(x.private.storage_proof.proof) for x in xs)
    return {"inputs": n, "nodes_hashed": nodes, "permutations": 24 * nodes + 8 * n,
            "verdicts_not_ok": int((dev[0] != 0).sum()), "ms": {k: _stats(v) for k, v in rows.items()}}


def bench_prove(prover, xs, reps):
    want = prover.prove_inputs(xs)  # warm-up
    got, statuses = prover.prove_inputs(xs, on_bad="skip")
    assert got == want and all(s.status == 0 for s in statuses)
    plain, skip = [], []
    for _ in range(reps):
        plain.append(_ms(lambda: prover.prove_inputs(xs))[0])
        skip.append(_ms(lambda: prover.prove_inputs(xs, on_bad="skip"))[0])
    return {"inputs": len(xs), "ms": {"prove_inputs": _stats(plain), "prove_inputs_skip": _stats(skip)}}


def find_bad_by_retries(qp, prover, xs):
    """today: prove, drop the one input the error names, prove again"""
    live, bad = list(range(len(xs))), []
    while True:
        try:
            return prover.prove_inputs([xs[i] for i in live]), bad
        except qp.QpError as e:
            m = re.search(r"proof (\d+)", str(e))
            off = re.search(r"batch offset (\d+)", str(e))
            at = int(m.group(1)) + (int(off.group(1)) if off and "device generator" in str(e) else 0)
            bad.append(live.pop(at))


def bench_three_bad(qp, prover, xs, reps):
    xs = list(xs)
    deep = [i for i, x in enumerate(xs) if x.private.storage_proof.proof]
    where = [deep[1], deep[len(deep) // 2], deep[-1]]
    for i in where:
        xs[i] = copy.deepcopy(xs[i])
        nodes = xs[i].private.storage_proof.proof
        nodes[-1] = nodes[-1][:5] + bytes([nodes[-1][5] ^ 1]) + nodes[-1][6:]
    proofs, bad = find_bad_by_retries(qp, prover, xs)  # warm-up, and the two ways' results compared
    got, statuses = prover.prove_inputs(xs, on_bad="skip")
    assert sorted(bad) == where == [i for i, s in enumerate(statuses) if s.status]
    assert [p for p in got if p is not None] == proofs
    retries, skip = [], []
    for _ in range(reps):
        retries.append(_ms(lambda: find_bad_by_retries(qp, prover, xs))[0])
        skip.append(_ms(lambda: prover.prove_inputs(xs, on_bad="skip"))[0])
    return {"inputs": len(xs), "bad_at": where, "passes_today": len(where) + 1,
            "ms": {"retries_today": _stats(retries), "one_skip_call": _stats(skip)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_bench.json"))
    a = ap.parse_args()
    import qp_wormhole as qp
    from qp_wormhole.synthetic import synthetic_inputs
    from libhash import lib_sha16
    ctx = qp.Context(0)
    circ = qp.Circuit.wormhole()
    xs = [synthetic_inputs(k) for k in range(a.n)]
    out = {"lib": lib_sha16(qp._native.LIB_PATH), "batch": a.n, "reps": a.reps}
    out["screen"] = bench_screen(qp, ctx, xs, a.reps)
    print(json.dumps(out["screen"]), flush=True)
    prover = qp.Prover(ctx, circ, max_batch=a.n)
    out["prove"] = bench_prove(prover, xs, a.reps)
    print(json.dumps(out["prove"]), flush=True)
    out["three_bad"] = bench_three_bad(qp, prover, xs, a.reps)
    print(json.dumps(out["three_bad"]), flush=True)
    prover.free()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
