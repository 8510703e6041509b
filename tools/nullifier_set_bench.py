"""Times the nullifier-set commitment at N = 2^20 admitted, credited transfers in a
ledger of capacity N + 1024: `commit_nullifiers` from scratch, again after 1024
more entries (the set is rebuilt whole), and the proofs of 1024 and of 65536 keys
(half members, half absent; the raw qp_ledger_set_proofs call into arrays made
beforehand).  Each figure is taken on the device path beside the host path of
the same library (ctx None), and beside `commit_log` from empty at the same
size as a scale.  A host clock around calls that end in a stream synchronise;
medians of --reps runs on fresh ledgers after one warm-up run; the host path,
which hashes two permutations per member on one thread (tens of seconds at
2^20), runs --host-reps times with no warm-up.  The two paths' roots and proofs
are compared as well.

The device path also records the split per kernel (qp_nullifier_set_times, HIP
events): select, tile sort, every merge pass, leaves, levels, and the sort's
achieved bytes/s against the 36 B x 2 per element a pass moves.

Each path runs in a child process of its own under `timeout`; the run stops at
the first child that fails.  Writes one JSON object (default
profiles/nullifier_set_bench.json) stamped with the library hash
(tools/libhash.py).  Needs an MI355X: without a device it fails.

  python tools/nullifier_set_bench.py [--log-n 20] [--reps 7] [--host-reps 2] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qp-zk-circuits-rm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 0xFFFFFFFF00000001
LEDGER_ROOT = [5, 6, 7, 8]
MORE = 1024


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def make_pis(rng, n):
    pis = np.zeros((n, 16), np.uint64)
    pis[:, 0:4] = rng.integers(0, P, size=(n, 4), dtype=np.uint64)
    pis[:, 4:8] = LEDGER_ROOT
    pis[:, 11] = 1
    pis[:, 12:16] = rng.integers(0, 1 << 16, size=(n, 1), dtype=np.uint64)
    return pis


def raw_proofs(L, h, q, bufs):
    k = len(q)
    found, pos, key, seq, sib, bits, depth, root, m = bufs
    args = [h.h, q.ctypes.data, k, found.ctypes.data, pos.ctypes.data]
    for s in range(2):
        args += [key[s].ctypes.data, seq[s].ctypes.data, sib[s].ctypes.data, bits[s].ctypes.data, depth[s].ctypes.data]
    rc = L.qp_ledger_set_proofs(*args, root.ctypes.data, ctypes.byref(m))
    assert rc == 0, L.qp_ledger_last_error(h.h)


def proof_bufs(k):
    return (np.zeros(k, np.uint8), np.zeros(k, np.uint64), [np.zeros((k, 4), np.uint64) for _ in range(2)],
            [np.zeros(k, np.uint64) for _ in range(2)], [np.zeros((k, 32, 4), np.uint64) for _ in range(2)],
            [np.zeros(k, np.uint32) for _ in range(2)], [np.zeros(k, np.uint32) for _ in range(2)],
            np.zeros(4, np.uint64), ctypes.c_uint64())


def run_path(device, log_n, reps):
    import qp_wormhole
    L = qp_wormhole.lib()
    ctx = qp_wormhole.Context(0) if device else None
    n = 1 << log_n
    rng = np.random.default_rng(20)
    pis, more = make_pis(rng, n), make_pis(rng, MORE)
    queries = {k: np.concatenate([pis[rng.integers(0, n, k // 2), 0:4], rng.integers(0, P, size=(k - k // 2, 4),
                                                                                   dtype=np.uint64)]) for k in (1024, 65536)}
    rows = {name: [] for name in ("commit_log_ms", "commit_set_ms", "commit_set_after_1024_ms", "proofs_1024_ms",
                                  "proofs_65536_ms")}
    stages, result = [], {}
    warmup = 1 if device else 0
    for rep in range(reps + warmup):
        h = qp_wormhole.WormholeLedger(ctx, [LEDGER_ROOT], capacity=n + MORE)
        st = h.cast_public(pis, raw=True)["status"]
        assert not st.any()
        out = {}

        def timed(name, call):
            t0 = time.perf_counter()
            v = call()
            out[name] = (time.perf_counter() - t0) * 1e3
            return v

        timed("commit_log_ms", h.commit_log)
        c0 = timed("commit_set_ms", h.commit_nullifiers)
        t = qp_wormhole.nullifier_set_times() if device else None
        assert not h.cast_public(more, raw=True)["status"].any()
        c1 = timed("commit_set_after_1024_ms", h.commit_nullifiers)
        assert c0[1] == n and c1[1] == n + MORE
        for k, q in queries.items():
            bufs = proof_bufs(k)
            timed(f"proofs_{k}_ms", lambda: raw_proofs(L, h, q, bufs))
            if k == 1024:
                result["proofs_1024_digest"] = [int(bufs[0].sum()), int(bufs[1].sum() % (1 << 62)),
                                                int(bufs[4][1].sum(dtype=np.uint64))]
        result["root"], result["root_after_1024"] = c0[0], c1[0]
        h.free()
        if rep >= warmup:  # the device path's first run is the warm-up
            for name in rows:
                rows[name].append(out[name])
            if t:
                stages.append(t)
    result.update({name: _stats(v) for name, v in rows.items()})
    if stages:
        med = lambda f: statistics.median(f(t) for t in stages)  # noqa: E731
        passes = len(stages[0]["merge_pass_ms"])
        split = {"select_ms": med(lambda t: t["select_ms"]), "tile_sort_ms_with_host_wait": med(lambda t: t["tile_sort_ms"]),
                 "merge_pass_ms": [med(lambda t, p=p: t["merge_pass_ms"][p]) for p in range(passes)],
                 "duplicates_and_leaves_ms": med(lambda t: t["leaves_ms"]), "levels_ms": med(lambda t: t["levels_ms"])}
        moved = n * 72
        split["merge_pass_GBps"] = [moved / (ms * 1e-3) / 1e9 for ms in split["merge_pass_ms"]]
        split["tile_sort_GBps_lower_bound"] = moved / (split["tile_sort_ms_with_host_wait"] * 1e-3) / 1e9
        result["device_split"] = split
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nullifier_set_bench.json"))
    ap.add_argument("--step", choices=["device", "host"])
    ap.add_argument("--step-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.step:
        with open(a.out, "w") as f:
            json.dump(run_path(a.step == "device", a.log_n, a.reps), f)
        return
    from libhash import lib_sha16
    res = {"n": 1 << a.log_n, "reps": a.reps, "host_reps": a.host_reps, "lib": lib_sha16()}
    for step in ("device", "host"):
        with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--log-n", str(a.log_n), "--reps", str(a.reps if step == "device" else a.host_reps), "--out", tmp.name]
            rc = subprocess.call(cmd)
            if rc:
                sys.exit(f"step {step} ended with {rc}; nothing further is started")
            res[step] = json.load(open(tmp.name))
    d, h = res["device"], res["host"]
    res["paths_agree"] = all(d[k] == h[k] for k in ("root", "root_after_1024", "proofs_1024_digest"))
    res["device_over_host"] = {k: d[k]["median"] / h[k]["median"] for k in d if k.endswith("_ms")}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("n", "paths_agree", "device_over_host")}))
    print(json.dumps(d.get("device_split")))
    if not res["paths_agree"]:
        sys.exit("the device and the host path disagree")


if __name__ == "__main__":
    main()
