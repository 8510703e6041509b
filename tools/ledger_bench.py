"""Times the transfer ledger: N = 2^20 synthetic transfers over 2^16 exit accounts
cast through cast_public into a ledger of capacity N, in batches of 256 (one
aggregated root's worth), 65536 and N, all distinct and with a quarter of them
double spends.  Per figure the wall time (a host clock around the calls; each
ends in a stream synchronise) and, on the device, the HIP-event times of the
upload and of screen to credit (qp_ledger_cast_times), medians of --reps runs
on fresh ledgers after one warm-up run.

The yardstick is the host path of the same library (ctx None: the sequential
tables of csrc/ledger_table.h) on the same stream in the same process.  The two
paths' results, payouts and recounts are compared as well.

Then, on the full log: reserve N -> 2 N, payouts (2^16 accounts), find of 65536
nullifiers (half of them absent), recount; and `cast` of 256 real Wormhole
proofs beside `verify_batch` alone on the same proofs.

The log commitment (first, `--only-log` for these rows alone), on a stream of
N + 256 + 65536 transfers, a quarter of them double spends: `commit_log` from
empty on the first N entries, again after 256 and after 65536 more, `receipts`
of 1024 entries (the Python call, and the two entry points under it alone), and
`audit_ledger_log` of the whole log with root, totals, payouts and two earlier
commitments, its arguments being arrays made beforehand; device beside host
(--host-reps runs: the host path hashes three permutations per entry on one
thread), results compared.

Restore and payout rounds (`--only-restore` for these rows alone, key
`restore_rounds`), on a log of N entries, a quarter of them double spends:
`restore` with and without an expected root beside the only alternative there
was, cast_public of the rebuilt public inputs into a fresh ledger plus
commit_log (which needs each entry's storage root: a published log does not
carry it); payouts_between of the last 256, the last 65536 and the whole log
beside the cumulative payouts(); the log-only form of the last 65536.  The host
path's root-expected restore runs on the first 2^16 entries (scaled).

Last, with --parent-lib FILE (the parent commit's libqpgpu.so), the path this
work must not disturb: the six cast_public rows, device and host path, on the
parent's library and on this one, both loaded into this process through plain
ctypes on the entry points both have, their runs alternating.  This library's
median of --reps runs has to lie inside the min-max of the parent's own runs on
every row; the figures are written first, then a miss fails the run.

Writes one JSON object (default profiles/ledger_bench.json) stamped with the
library hash (tools/libhash.py).  Needs an MI355X: without a device it fails.

  python tools/ledger_bench.py [--log-n 20] [--reps 5] [--proofs 256] [--only-log] [--only-restore] [--parent-lib FILE] [--out FILE]
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


def log_commitment(qp, ctx, pis, n, reps):
    """commit_log from empty on the first n entries of the stream and after batches of 256 and 65536
    more, receipts of 1024 entries, and the audit of the whole log with every claim: wall medians on
    one path.  The audit's log and claims are the arrays the ABI takes, made outside the timed call;
    receipts_1024 is the Python call, its 1024 TransferReceipt objects included, receipts_1024_abi the
    two entry points under it (qp_ledger_receipts, qp_ledger_entries_at) on buffers made beforehand"""
    import ctypes
    assert len(pis) == n + 256 + 65536
    t = {k: [] for k in ("commit_from_empty", "commit_after_256", "commit_after_65536", "receipts_1024",
                         "receipts_1024_abi", "audit")}
    seqs = np.random.default_rng(3).integers(0, n, 1024).astype(np.uint64)
    L, last = qp.lib(), None

    def timed(key, fn):
        t0 = time.perf_counter()
        out = fn()
        t[key].append(time.perf_counter() - t0)
        return out
    for _ in range(reps + 1):  # the first run is the warm-up
        led = qp.WormholeLedger(ctx, ROOTS, capacity=len(pis))
        led.cast_public(pis[:n], reserve=False, raw=True)
        first = timed("commit_from_empty", led.commit_log)
        rs = timed("receipts_1024", lambda: led.receipts(seqs))
        assert all(qp.WormholeLedger.check_receipt(r) for r in rs[:8])
        sib, bits, depth = np.zeros((1024, 32, 4), np.uint64), np.zeros(1024, np.uint32), np.zeros(1024, np.uint32)
        root, m = np.zeros(4, np.uint64), ctypes.c_uint64()
        nul, acc = np.zeros((1024, 4), np.uint64), np.zeros((1024, 4), np.uint64)
        num, amt, fl = np.zeros(1024, np.uint64), np.zeros((1024, 4), np.uint32), np.zeros(1024, np.uint8)
        assert timed("receipts_1024_abi", lambda: (
            L.qp_ledger_receipts(led.h, seqs.ctypes.data, 1024, sib.ctypes.data, bits.ctypes.data, depth.ctypes.data,
                                 None, root.ctypes.data, ctypes.byref(m)),
            L.qp_ledger_entries_at(led.h, seqs.ctypes.data, 1024, nul.ctypes.data, num.ctypes.data, amt.ctypes.data,
                                   acc.ctypes.data, fl.ctypes.data))) == (0, 0)
        assert sib[0, :depth[0]].tolist() == rs[0].siblings and int(bits[0]) == rs[0].path_bits
        led.cast_public(pis[n:n + 256], reserve=False, raw=True)
        timed("commit_after_256", led.commit_log)
        led.cast_public(pis[n + 256:], reserve=False, raw=True)
        root, m = timed("commit_after_65536", led.commit_log)
        nul, acc = np.zeros((m, 4), np.uint64), np.zeros((m, 4), np.uint64)
        num, amt, fl = np.zeros(m, np.uint64), np.zeros((m, 4), np.uint32), np.zeros(m, np.uint8)
        assert L.qp_ledger_entries(led.h, 0, m, nul.ctypes.data, num.ctypes.data, amt.ctypes.data, acc.ctypes.data,
                                   fl.ctypes.data) == 0
        payouts, (credited, _, total) = led.payouts(raw=True), led.recount()
        earlier = [(first[0], first[1]), (led.root_at(m // 2 + 1), m // 2 + 1)]
        led.free()
        rep = timed("audit", lambda: qp.audit_ledger_log(ctx, (nul, num, amt, acc, fl), root, (credited, total),
                                                         payouts, earlier))
        assert rep.status == 0, rep
        last = (root, m, first, [tuple(r) for r in rs[:8]], tuple(rep))
    return {"entries_at_first_commit": n, "entries": len(pis), "accounts_paid": len(payouts[2]),
            **{k: _stats(v[1:]) for k, v in t.items()}}, last


class PlainLedgerLib:
    """the entry points of the cast path, which the parent's library has too, through plain ctypes"""

    def __init__(self, path, device):
        import ctypes
        from libhash import lib_sha16
        VP, U64 = ctypes.c_void_p, ctypes.c_uint64
        self.path, self.sha, self.ct = path, lib_sha16(path), ctypes
        self.L = L = ctypes.CDLL(path)
        L.qp_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(VP)]
        L.qp_ctx_destroy.argtypes, L.qp_ctx_destroy.restype = [VP], None
        L.qp_ledger_new.argtypes = [VP, VP, ctypes.c_uint32, VP, U64, ctypes.POINTER(VP)]
        L.qp_ledger_free.argtypes, L.qp_ledger_free.restype = [VP], None
        L.qp_ledger_cast_public.argtypes = [VP, VP, VP, ctypes.c_uint32, VP]
        L.qp_ledger_recount.argtypes = [VP, VP]
        L.qp_ledger_cast_times.argtypes = [VP, ctypes.POINTER(ctypes.c_double)]
        self.ctx = None
        if device:
            self.ctx = VP()
            assert L.qp_ctx_create(0, ctypes.byref(self.ctx)) == 0

    def run(self, pis, batch):
        """one fresh ledger, the stream in batches of `batch`: (wall, upload ms, kernels ms, results, recount)"""
        ct, L, n = self.ct, self.L, len(pis)
        led, roots = ct.c_void_p(), np.array(ROOTS, np.uint64)
        assert L.qp_ledger_new(self.ctx, roots.ctypes.data, len(ROOTS), None, n, ct.byref(led)) == 0
        res, ms, u, k = np.zeros((n, 3), np.uint64), (ct.c_double * 2)(), 0.0, 0.0  # qp_transfer_result: 24 bytes
        t0 = time.perf_counter()
        for at in range(0, n, batch):
            assert L.qp_ledger_cast_public(led, pis[at:at + batch].ctypes.data, None, len(pis[at:at + batch]),
                                           res[at:at + batch].ctypes.data) == 0
            if self.ctx is not None:
                assert L.qp_ledger_cast_times(led, ms) == 0
                u, k = u + ms[0], k + ms[1]
        wall = time.perf_counter() - t0
        rec = np.zeros(6, np.uint64)
        assert L.qp_ledger_recount(led, rec.ctypes.data) == 0
        L.qp_ledger_free(led)
        return wall, u, k, res, rec.tolist()

    def close(self):
        if self.ctx is not None:
            self.L.qp_ctx_destroy(self.ctx)
            self.ctx = None


def ab_cast_public(parent_path, this_path, n, reps):
    """the cast_public rows on the parent's library and on this one, both loaded into this process:
    per row and path the runs alternate between the two libraries (which one goes first swaps with
    every run; one warm-up run each is dropped), and this library's median wall time has to lie
    inside the min-max of the parent's own runs"""
    rows, misses = [], []
    for path_name, device in (("device", True), ("host", False)):
        libs = {"parent": PlainLedgerLib(parent_path, device), "this": PlainLedgerLib(this_path, device)}
        for name, doubles in (("distinct", 0), ("quarter_doubles", n // 4)):
            pis = make_stream(np.random.default_rng(1), n, doubles)
            for batch in (256, 65536, n):
                runs = {k: {"wall_s": [], "upload_ms": [], "kernels_ms": []} for k in libs}
                for rep in range(reps + 1):
                    got = {}
                    for label in (("parent", "this"), ("this", "parent"))[rep & 1]:
                        wall, u, k, res, rec = libs[label].run(pis, batch)
                        got[label] = (res, rec)
                        if rep:
                            runs[label]["wall_s"].append(wall)
                            runs[label]["upload_ms"].append(u), runs[label]["kernels_ms"].append(k)
                    same = bool((got["parent"][0] == got["this"][0]).all()) and got["parent"][1] == got["this"][1]
                    assert same, "the parent's library and this one disagree"
                row = {"path": path_name, "stream": name, "batch": min(batch, n), "results_equal": True}
                for label in libs:
                    keys = ("wall_s", "upload_ms", "kernels_ms") if device else ("wall_s",)
                    row[label] = {k: _stats(runs[label][k]) for k in keys}
                    row[label]["wall_runs_s"] = runs[label]["wall_s"]
                lo, hi, med = row["parent"]["wall_s"]["min"], row["parent"]["wall_s"]["max"], row["this"]["wall_s"]["median"]
                row["this_median_over_parent_median"] = med / row["parent"]["wall_s"]["median"]
                row["this_median_inside_parent_range"] = bool(lo <= med <= hi)
                if not row["this_median_inside_parent_range"]:
                    misses.append("%s %s batch %d: %.6f s outside [%.6f, %.6f]" % (path_name, name, batch, med, lo, hi))
                rows.append(row)
                print(json.dumps(row), flush=True)
        shas = {k: v.sha for k, v in libs.items()}
        for v in libs.values():
            v.close()
    return {"what": "cast_public of the whole stream into a fresh ledger per run, both libraries in one process "
                    "through plain ctypes, runs alternating between them, one warm-up run each dropped; wall: "
                    "perf_counter around the calls; *_ms: HIP events summed over the calls",
            "parent_library": shas["parent"], "library": shas["this"], "reps": reps, "rows": rows,
            "all_medians_inside_parent_range": not misses}, misses


def restore_rounds(qp, ctx, pis, reps, root_n=None):
    """On one path, over the log the stream `pis` leaves (the publisher is a ledger of the same path):
    `restore` with and without an expected root; the only way back to a live ledger before restore
    existed: cast_public of the rebuilt public inputs into a fresh ledger, plus commit_log (it needs
    each entry's storage root, which a published log does not carry: the stream's own are used);
    payouts_between of the last 256, the last 65536 and the whole log beside the cumulative payouts();
    and the log-only form of the last 65536.  Wall medians of `reps` runs after one warm-up.  root_n:
    the root-expected restore (and the alternative, which commits) on the first root_n entries only,
    for the host path, which hashes three permutations per entry on one thread."""
    n_pis = len(pis)
    led = qp.WormholeLedger(ctx, ROOTS, capacity=n_pis)
    led.cast_public(pis, reserve=False, raw=True)
    n = led.admitted
    entries = led._entries_at(np.arange(n, dtype=np.uint64))  # the arrays the ABI takes, made beforehand
    root_n = n if root_n is None else min(root_n, n)
    root_at = led.root_at(root_n)
    cast_count = led.cast_count
    want = (led.payouts(raw=True), led.recount())
    short = tuple(a[:root_n] for a in entries)
    short_pis = pis[:root_n]  # every transfer of the stream is admitted, so entry i is transfer i
    assert n == n_pis and (entries[0][:root_n] == short_pis[:, 0:4]).all()
    t = {k: [] for k in ("restore", "restore_with_root", "recast_and_commit", "payouts_between_last_256",
                         "payouts_between_last_65536", "payouts_between_whole", "payouts_cumulative",
                         "log_payouts_last_65536")}

    def timed(key, fn):
        t0 = time.perf_counter()
        out = fn()
        t[key].append(time.perf_counter() - t0)
        return out
    last = None
    for _ in range(reps + 1):
        again = timed("restore", lambda: qp.WormholeLedger.restore(ctx, ROOTS, entries, cast_count=cast_count, capacity=n))
        got = (again.payouts(raw=True), again.recount())
        assert all((a == b).all() for a, b in zip(got[0], want[0])) and got[1] == want[1]
        again.free()
        again = timed("restore_with_root", lambda: qp.WormholeLedger.restore(ctx, ROOTS, short, capacity=root_n,
                                                                              root=root_at))
        assert again.commit_log() == (root_at, root_n)
        again.free()

        def recast():
            fresh = qp.WormholeLedger(ctx, ROOTS, capacity=root_n)
            fresh.cast_public(short_pis, reserve=False, raw=True)
            return fresh, fresh.commit_log()
        fresh, pair = timed("recast_and_commit", recast)
        assert pair == (root_at, root_n)
        fresh.free()
        rows = {}
        for key, m0 in (("payouts_between_last_256", n - 256), ("payouts_between_last_65536", n - 65536),
                        ("payouts_between_whole", 0)):
            rows[key] = timed(key, lambda: led.payouts_between(m0, n, raw=True))
        # after the warm-up the ledger keeps its payee list, so these are the gathers alone; the first call's
        # compaction of the whole log is full_log's `payouts` row
        cumulative = timed("payouts_cumulative", lambda: led.payouts(raw=True))
        assert all((a == b).all() for a, b in zip(rows["payouts_between_whole"], cumulative))
        log_rows = timed("log_payouts_last_65536", lambda: qp.ledger_log_payouts(ctx, entries, n - 65536, n, raw=True))
        assert all((a == b).all() for a, b in zip(log_rows, rows["payouts_between_last_65536"]))
        last = ([x.tolist() for x in rows["payouts_between_last_256"]], len(rows["payouts_between_last_65536"][2]),
                len(cumulative[2]), root_at)
    led.free()
    rec = {k: _stats(v[1:]) for k, v in t.items()}
    rec.update({"entries": n, "root_entries": root_n, "accounts": last[2], "accounts_last_65536": last[1],
                "accounts_last_256": len(last[0][2])})
    return rec, last


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
    ap.add_argument("--host-reps", type=int, default=3, help="runs of the host path's log-commitment rows")
    ap.add_argument("--proofs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_bench.json"))
    ap.add_argument("--only-log", action="store_true",
                    help="only the log commitment's rows (and the A/B, if asked for), merged into an existing --out file")
    ap.add_argument("--only-restore", action="store_true",
                    help="only the restore and payout-round rows (and the A/B, if asked for), merged into an existing --out file")
    ap.add_argument("--parent-lib", help="the parent commit's libqpgpu.so: the cast_public rows on both libraries")
    a = ap.parse_args()
    import qp_wormhole as qp
    from qp_wormhole._native import LIB_PATH
    from libhash import lib_sha16
    ctx = qp.Context(0)
    n = 1 << a.log_n
    out = {"library": lib_sha16(), "transfers": n, "accounts": ACCOUNTS, "reps": a.reps, "cast_public": []}
    if (a.only_log or a.only_restore) and os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    if not a.only_log:
        pis = make_stream(np.random.default_rng(1), n, n // 4)
        dev, dlast = restore_rounds(qp, ctx, pis, a.reps)
        host, hlast = restore_rounds(qp, None, pis, a.reps, root_n=1 << 16)
        out["restore_rounds"] = {
            "library": lib_sha16(), "stream": "quarter_doubles", "device": dev, "host": host,
            "what": "wall of one call (perf_counter), medians of reps runs after one warm-up; the log's arrays are "
                    "made before the timed calls; host.restore_with_root and host.recast_and_commit are scaled: the "
                    "first host.root_entries entries only; recast_and_commit needs each entry's storage root, which "
                    "a published log does not carry; payouts_cumulative is the gathers alone (the payee list is "
                    "kept from the warm-up; full_log.payouts is a first call)",
            "results_equal": dlast[:3] == hlast[:3],
            "device_wall_over_host_wall": {k: dev[k]["median"] / host[k]["median"] for k in dev
                                           if isinstance(dev[k], dict) and k not in ("restore_with_root",
                                                                                     "recast_and_commit")}}
        print(json.dumps(out["restore_rounds"]), flush=True)
        assert dlast[:3] == hlast[:3]
    if not a.only_restore:
        pis = make_stream(np.random.default_rng(1), n + 256 + 65536, (n + 256 + 65536) // 4)
        dev, dlast = log_commitment(qp, ctx, pis, n, a.reps)
        host, hlast = log_commitment(qp, None, pis, n, a.host_reps)
        out["log_commitment"] = {"library": lib_sha16(), "stream": "quarter_doubles", "device": dev, "host": host,
                                 "results_equal": dlast == hlast,
                                 "device_wall_over_host_wall": {k: dev[k]["median"] / host[k]["median"] for k in dev
                                                                if isinstance(dev[k], dict)}}
        print(json.dumps(out["log_commitment"]), flush=True)
        assert dlast == hlast
    for name, doubles in (() if a.only_log or a.only_restore else (("distinct", 0), ("quarter_doubles", n // 4))):
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
    if a.proofs and not a.only_log and not a.only_restore:
        out["real_proofs"] = real_proofs(qp, ctx, a.proofs, a.reps)
        print(json.dumps(out["real_proofs"]), flush=True)
    misses = []
    out.setdefault("ab_cast_public", "not measured")
    if a.parent_lib:
        out["ab_cast_public"], misses = ab_cast_public(os.path.abspath(a.parent_lib), LIB_PATH, n, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    # the figures are on record either way; a median outside the parent's own spread fails the run
    assert not misses, "cast_public medians outside the parent's min-max: " + "; ".join(misses)


if __name__ == "__main__":
    main()
