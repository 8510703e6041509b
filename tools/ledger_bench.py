"""Times the transfer ledger: N = 2^20 synthetic transfers over 2^16 exit accounts
cast through cast_public into a ledger of capacity N, in batches of 256 (one
aggregated root's worth), 65536 and N, all distinct and with a quarter of them
double spends.  Per figure the wall time (a host clock around the calls; each
ends in a stream synchronise) and, on the device, the HIP-event times of the
upload and of screen to credit (qp_ledger_cast_times), medians of --reps runs
on fresh ledgers after one warm-up run.

The yardstick is the host path of the same library (ctx None: the sequential
tables of csrc/ledger_table.h) on the same stream in the same process; there is
no parent figure, the parent has no ledger.  The two paths' results, payouts and
recounts are compared as well.

Then, on the full log: reserve N -> 2 N, payouts (2^16 accounts), find of 65536
nullifiers (half of them absent), recount; and `cast` of 256 real Wormhole
proofs beside `verify_batch` alone on the same proofs.

Writes one JSON object (default profiles/ledger_bench.json) stamped with the
library hash (tools/libhash.py).  Needs an MI355X: without a device it fails.

  python tools/ledger_bench.py [--log-n 20] [--reps 5] [--proofs 256] [--out FILE]
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
ROOTS = [[5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]]
ACCOUNTS = 1 << 16


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def make_stream(rng, n, doubles):
    """pis [n][16]: n - doubles distinct nullifiers, then `doubles` copies of earlier ones (with other
    amounts and accounts), shuffled; roots among ROOTS, random 32-bit limbs, 2^16 accounts"""
    pis = np.zeros((n, 16), np.uint64)
    fresh = n - doubles
    pis[:fresh, 0:4] = rng.integers(0, P, size=(fresh, 4), dtype=np.uint64)
    pis[fresh:, 0:4] = pis[rng.integers(0, fresh, doubles), 0:4]
    pis[:, 4:8] = np.array(ROOTS, np.uint64)[rng.integers(0, len(ROOTS), n)]
    pis[:, 8:12] = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64)
    accounts = rng.integers(0, P, size=(ACCOUNTS, 4), dtype=np.uint64)
    pis[:, 12:16] = accounts[rng.integers(0, ACCOUNTS, n)]
    return np.ascontiguousarray(pis[rng.permutation(n)])


def cast_stream(Ledger, ctx, pis, batch, reps):
    """reps fresh ledgers, the stream in batches of `batch`: wall of all the casts, summed event times"""
    n = len(pis)
    wall, up, ker, last = [], [], [], None
    for rep in range(reps + 1):  # the first run is the warm-up
        led = Ledger(ctx, ROOTS, capacity=n)
        res, u, k = [], 0.0, 0.0
        t0 = time.perf_counter()
        for at in range(0, n, batch):
            res.append(led.cast_public(pis[at:at + batch], reserve=False, raw=True))
            if ctx is not None:
                ms = led.cast_times()
                u, k = u + ms["upload_ms"], k + ms["kernels_ms"]
        wall.append(time.perf_counter() - t0)
        up.append(u), ker.append(k)
        if rep == reps:
            last = (np.concatenate(res), led.payouts(), led.recount())
        led.free()
    rec = {"batch": batch, "calls": (n + batch - 1) // batch, "wall_s": _stats(wall[1:]),
           "transfers_per_s_wall": n / statistics.median(wall[1:])}
    if ctx is not None:
        rec["upload_ms"] = _stats(up[1:])
        rec["kernels_ms"] = _stats(ker[1:])
    return rec, last


def full_log(Ledger, ctx, pis, rng, reps):
    """reserve, payouts, find and recount on a ledger holding the whole stream: wall medians"""
    n = len(pis)
    t = {k: [] for k in ("reserve", "payouts", "find_65536", "recount")}
    q = np.ascontiguousarray(pis[rng.integers(0, n, 65536), 0:4])
    q[1::2] = rng.integers(0, P, size=(32768, 4), dtype=np.uint64)
    last = None
    for _ in range(reps):
        led = Ledger(ctx, ROOTS, capacity=n)
        led.cast_public(pis, reserve=False, raw=True)

        def timed(key, fn):
            t0 = time.perf_counter()
            out = fn()
            t[key].append(time.perf_counter() - t0)
            return out
        pay = [x.tolist() for x in timed("payouts", lambda: led.payouts(raw=True))]
        found = timed("find_65536", lambda: led.find(q, raw=True))
        rec = timed("recount", led.recount)
        timed("reserve", lambda: led.reserve(2 * n))
        assert [x.tolist() for x in led.payouts(raw=True)] == pay and (led.find(q, raw=True) == found).all() and led.recount() == rec
        last = (pay, found.tolist(), rec)
        led.free()
    return {k: _stats(v) for k, v in t.items()}, last


def real_proofs(qp, ctx, nproofs, reps):
    """`cast` of real Wormhole proofs on both paths beside `verify_batch` alone"""
    from qp_wormhole.prover import _verifier_only
    from qp_wormhole.synthetic import synthetic_inputs
    circ = qp.Circuit.wormhole()
    prover = qp.Prover(ctx, circ, max_batch=64)
    proofs = []
    for at in range(0, nproofs, 64):
        proofs += prover.prove_inputs([synthetic_inputs(at + i, (at + i) % 3) for i in range(min(64, nproofs - at))])
    ver = qp.WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=nproofs)
    roots = sorted({tuple(int.from_bytes(p[len(p) - 128 + 32 + 8 * j:len(p) - 128 + 40 + 8 * j], "little") for j in range(4))
                    for p in proofs})
    t = {"verify_batch": [], "cast_device": [], "cast_host": []}
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        verdicts = ver.verify_batch(proofs)
        t["verify_batch"].append(time.perf_counter() - t0)
        assert not any(verdicts)
        res = {}
        for key, c in (("cast_device", ctx), ("cast_host", None)):
            led = qp.WormholeLedger(c, [list(r) for r in roots], verifier=ver, capacity=nproofs)
            t0 = time.perf_counter()
            out = led.cast(proofs, reserve=False, raw=True)
            t[key].append(time.perf_counter() - t0)
            res[key] = (out.tolist(), led.payouts())
            led.free()
        assert res["cast_device"] == res["cast_host"]
    credited = sum(1 for r in res["cast_device"][0] if r[0] == 0)
    ver.close()
    prover.free()
    return {"proofs": nproofs, "credited": credited, **{k: _stats(v[1:]) for k, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_bench.json"))
    a = ap.parse_args()
    import qp_wormhole as qp
    from libhash import lib_sha16
    ctx = qp.Context(0)
    n = 1 << a.log_n
    out = {"library": lib_sha16(), "transfers": n, "accounts": ACCOUNTS, "reps": a.reps, "cast_public": []}
    for name, doubles in (("distinct", 0), ("quarter_doubles", n // 4)):
        pis = make_stream(np.random.default_rng(1), n, doubles)
        for batch in (256, 65536, n):
            dev, dlast = cast_stream(qp.WormholeLedger, ctx, pis, batch, a.reps)
            host, hlast = cast_stream(qp.WormholeLedger, None, pis, batch, a.reps)
            same = bool((dlast[0] == hlast[0]).all()) and dlast[1:] == hlast[1:]
            out["cast_public"].append({"stream": name, "device": dev, "host": host, "results_equal": same,
                                       "credited": dlast[2][0], "admitted": dlast[2][1], "accounts": len(dlast[1])})
            print(json.dumps(out["cast_public"][-1]), flush=True)
            assert same
        if name == "quarter_doubles":
            dev, dlast = full_log(qp.WormholeLedger, ctx, pis, np.random.default_rng(2), a.reps)
            host, hlast = full_log(qp.WormholeLedger, None, pis, np.random.default_rng(2), a.reps)
            out["full_log"] = {"device": dev, "host": host, "results_equal": dlast == hlast}
            print(json.dumps(out["full_log"]), flush=True)
            assert dlast == hlast
    if a.proofs:
        out["real_proofs"] = real_proofs(qp, ctx, a.proofs, a.reps)
        print(json.dumps(out["real_proofs"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
