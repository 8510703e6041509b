"""Times the payout claims commitment on two ledgers of N = 2^20 credited transfers:
`exits` pays 2^16 exit accounts (the ledger bench's workload) and `distinct` pays
N distinct accounts, where the sort dominates.  Rows: `commit_claims` over the
whole log, over a round of the last 65536 entries, the claims of 1024 and of
65536 accounts (half payees, half absent; the raw qp_ledger_claims call into
arrays made beforehand) and `ledger_log_claims_root` of the full log.  Each
figure is taken on the device path beside the host path of the same library
(ctx None; one run, labelled so).  A host clock around calls that end in a
stream synchronise; medians of --reps runs on fresh ledgers after one warm-up
run, with min and max.  The device path also records the stage split
(qp_ledger_claims_times, HIP events) of the cumulative commit.  The two paths'
roots, totals and claims are compared as well.

Each path runs in a child process of its own under `timeout`; the run stops at
the first child that fails.  Writes one JSON object (default
profiles/claims_bench.json) stamped with the library hash (tools/libhash.py).
Needs an MI355X: without a device it fails.

  python tools/claims_bench.py [--log-n 20] [--reps 7] [--out FILE]
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
ROUND = 65536


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def make_pis(rng, n, workload):
    pis = np.zeros((n, 16), np.uint64)
    pis[:, 0:4] = rng.integers(0, P, size=(n, 4), dtype=np.uint64)
    pis[:, 4:8] = LEDGER_ROOT
    pis[:, 8:12] = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64)
    if workload == "exits":
        pis[:, 12:16] = rng.integers(0, 1 << 16, size=(n, 1), dtype=np.uint64)
    else:
        pis[:, 12:16] = rng.integers(0, P, size=(n, 4), dtype=np.uint64)
    return pis


def claim_bufs(k):
    two = lambda shape, dt: [np.zeros(shape, dt) for _ in range(2)]  # noqa: E731
    return (np.zeros(k, np.uint8), np.zeros(k, np.uint64), two((k, 4), np.uint64), two((k, 5), np.uint32),
            two(k, np.uint64), two((k, 32, 4), np.uint64), two(k, np.uint32), two(k, np.uint32), np.zeros(4, np.uint64),
            ctypes.c_uint64())


def raw_claims(L, h, m0, m1, q, bufs):
    found, pos, acc, tot, seq, sib, bits, depth, root, count = bufs
    args = [h.h, m0, m1, q.ctypes.data, len(q), found.ctypes.data, pos.ctypes.data]
    for s in range(2):
        args += [acc[s].ctypes.data, tot[s].ctypes.data, seq[s].ctypes.data, sib[s].ctypes.data, bits[s].ctypes.data,
                 depth[s].ctypes.data]
    rc = L.qp_ledger_claims(*args, root.ctypes.data, ctypes.byref(count))
    assert rc == 0, L.qp_ledger_last_error(h.h)


def raw_entries(L, h, n):
    nul, acc = np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64)
    num, amt, fl = np.zeros(n, np.uint64), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint8)
    assert L.qp_ledger_entries(h.h, 0, n, nul.ctypes.data, num.ctypes.data, amt.ctypes.data, acc.ctypes.data,
                               fl.ctypes.data) == 0
    return nul, num, amt, acc, fl


def run_workload(device, workload, log_n, reps):
    import qp_wormhole
    L = qp_wormhole.lib()
    ctx = qp_wormhole.Context(0) if device else None
    n = 1 << log_n
    rng = np.random.default_rng(17)
    pis = make_pis(rng, n, workload)
    queries = {k: np.concatenate([pis[rng.integers(0, n, k // 2), 12:16], rng.integers(0, P, size=(k - k // 2, 4),
                                                                                     dtype=np.uint64)]) for k in (1024, 65536)}
    names = ("commit_claims_ms", "commit_claims_round_65536_ms", "claims_1024_ms", "claims_65536_ms", "log_claims_root_ms")
    rows = {name: [] for name in names}
    stages, result = [], {}
    warmup = 1 if device else 0
    for rep in range(reps + warmup):
        h = qp_wormhole.WormholeLedger(ctx, [LEDGER_ROOT], capacity=n)
        assert not h.cast_public(pis, raw=True)["status"].any()
        out = {}

        def timed(name, call):
            t0 = time.perf_counter()
            v = call()
            out[name] = (time.perf_counter() - t0) * 1e3
            return v

        whole = timed("commit_claims_ms", h.commit_claims)
        t = qp_wormhole.claims_times() if device else None
        for k, q in queries.items():
            bufs = claim_bufs(k)
            timed(f"claims_{k}_ms", lambda: raw_claims(L, h, 0, n, q, bufs))
            if k == 1024:
                result["claims_1024_digest"] = [int(bufs[0].sum()), int(bufs[1].sum() % (1 << 62)),
                                                int(bufs[5][1].sum(dtype=np.uint64)), int(bufs[3][1].sum(dtype=np.uint64))]
        rnd = timed("commit_claims_round_65536_ms", lambda: h.commit_claims(n - ROUND, n))
        log = raw_entries(L, h, n)
        got = timed("log_claims_root_ms", lambda: qp_wormhole.ledger_log_claims_root(ctx, log))
        assert got[:3] == (whole.root, whole.count, whole.total)
        result.update(root=whole.root, rows=whole.count, total=str(whole.total), round_root=rnd.root, round_rows=rnd.count)
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
        result["device_split"] = {
            "credit_and_compaction_ms_with_alloc_and_host_wait": med(lambda t: t["credit_ms"]),
            "tile_sort_ms": med(lambda t: t["tile_sort_ms"]),
            "merge_pass_ms": [med(lambda t, p=p: t["merge_pass_ms"][p]) for p in range(passes)],
            "leaves_and_total_ms": med(lambda t: t["leaves_ms"]), "levels_ms": med(lambda t: t["levels_ms"])}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "claims_bench.json"))
    ap.add_argument("--step", choices=["device", "host"])
    ap.add_argument("--workload", choices=["exits", "distinct"])
    ap.add_argument("--step-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.step:
        with open(a.out, "w") as f:
            json.dump(run_workload(a.step == "device", a.workload, a.log_n, a.reps), f)
        return
    from libhash import lib_sha16
    res = {"n": 1 << a.log_n, "reps": a.reps, "host_runs": 1, "lib": lib_sha16(), "workloads": {}}
    same = ("root", "rows", "total", "round_root", "round_rows", "claims_1024_digest")
    for workload in ("exits", "distinct"):
        w = res["workloads"][workload] = {}
        for step in ("device", "host"):
            with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                       "--workload", workload, "--log-n", str(a.log_n), "--reps", str(a.reps if step == "device" else 1),
                       "--out", tmp.name]
                rc = subprocess.call(cmd)
                if rc:
                    sys.exit(f"step {step} of {workload} ended with {rc}; nothing further is started")
                w[step] = json.load(open(tmp.name))
        d, h = w["device"], w["host"]
        w["paths_agree"] = all(d[k] == h[k] for k in same)
        w["device_over_host_one_run"] = {k: d[k]["median"] / h[k]["median"] for k in d if k.endswith("_ms")}
        print(json.dumps({"workload": workload, "paths_agree": w["paths_agree"],
                          "device_ms": {k: d[k]["median"] for k in d if k.endswith("_ms")},
                          "host_ms_one_run": {k: h[k]["median"] for k in h if k.endswith("_ms")}}))
        print(json.dumps(d.get("device_split")))
    nset = os.path.join(ROOT, "profiles", "nullifier_set_bench.json")
    if os.path.exists(nset):  # for scale: the same sort and tree work at the same member count, without the round credit
        ns = json.load(open(nset))
        res["commit_nullifiers_for_scale"] = {"n": ns.get("n"), "commit_set_ms": ns.get("device", {}).get("commit_set_ms"),
                                              "from": "profiles/nullifier_set_bench.json (an earlier run)"}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    if not all(w["paths_agree"] for w in res["workloads"].values()):
        sys.exit("the device and the host path disagree")


if __name__ == "__main__":
    main()
