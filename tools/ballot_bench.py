"""Times the ballot box: N = 2^20 synthetic ballots cast through cast_public into
a box of capacity 2 N, in batches of 1024, 65536 and N, all distinct and with a
quarter of them double votes; reserve 2 N -> 4 N on the full log; recount.
Per figure the wall time (a host clock around the calls; each ends in a stream
synchronise) and, on the device, the HIP-event times of the log upload and of
insert + resolve (qp_ballot_box_cast_times), medians of --reps runs.

The yardstick is the host path of the same library (ctx None: the sequential
table of csrc/ballot_table.h) on the same stream in the same process; there is
no earlier device counter to compare with.  The results of the two paths are
compared as well.

Then `cast` of 1024 real voting proofs beside `verify_batch` alone on the same
proofs: what the box adds to verification.

The log commitment, on a box of N distinct entries at capacity 2 N, device and
host path side by side: `commit_log` from empty, `commit_log` after one more
batch of 1024 and one of 65536, `find` of 1024 and of 65536 nullifiers (half of
them absent), `receipts` of 1024 entries.

The log audit, on a log of N honest entries (a quarter double votes):
`audit_log` with the root and the tally claimed, the same with 1024 earlier
commitments, `restore`, `roots_at` of 1024 sizes, and beside them what an
auditor could do before: `cast_public` of the log's public inputs into a fresh
box plus `commit_log`.  The host path of the same library runs at 2^16 entries
(--audit-host-log-n), with the device at that size next to it.  --audit-only
takes these records alone and puts them into the output file's `log_audit` key.

Last, with --parent-lib FILE, one A/B of the path this work must not disturb:
`cast_public`, distinct, 16 x 65536, in a fresh process per library (plain
ctypes on the entry points both libraries have), 7 runs each; the new median
should lie inside the parent's own min-max.

Writes one JSON object (default profiles/ballot_bench.json) stamped with the
library hash (tools/libhash.py).  Needs an MI355X: without a device it fails.

  python tools/ballot_bench.py [--log-n 20] [--reps 7] [--proofs 1024] [--parent-lib FILE] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qp-zk-circuits-rm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

P = 0xFFFFFFFF00000001
PROPOSAL = [0x2A2A2A2A2A2A2A2A] * 4
ROOT_DIGEST = [5, 6, 7, 8]


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def make_stream(rng, n, doubles):
    """pis [n][13]: n - doubles distinct nullifiers, then `doubles` copies of earlier ones, shuffled"""
    pis = np.zeros((n, 13), np.uint64)
    pis[:, 0:4] = PROPOSAL
    pis[:, 4:8] = ROOT_DIGEST
    pis[:, 8] = rng.integers(0, 2, n, dtype=np.uint64)
    fresh = n - doubles
    pis[:fresh, 9:13] = rng.integers(0, P, size=(fresh, 4), dtype=np.uint64)
    pis[fresh:, 9:13] = pis[rng.integers(0, fresh, doubles), 9:13]
    return np.ascontiguousarray(pis[rng.permutation(n)])


def cast_stream(BallotBox, ctx, pis, capacity, batch, reps):
    """reps fresh boxes, the stream in batches of `batch`: wall of all the casts, summed event times"""
    n = len(pis)
    wall, up, ir, last = [], [], [], None
    for _ in range(reps + 1):  # the first run is the warm-up
        box = BallotBox(ctx, PROPOSAL, [ROOT_DIGEST], capacity=capacity)
        res, u, k = [], 0.0, 0.0
        t0 = time.perf_counter()
        for at in range(0, n, batch):
            res.append(box.cast_public(pis[at:at + batch], reserve=False, raw=True))
            if ctx is not None:
                ms = box.cast_times()
                u, k = u + ms["upload_ms"], k + ms["insert_resolve_ms"]
        wall.append(time.perf_counter() - t0)
        up.append(u), ir.append(k)
        last = (np.concatenate(res), box.tally, box.recount())
        box.free()
    rec = {"batch": batch, "calls": (n + batch - 1) // batch, "wall_s": _stats(wall[1:]),
           "ballots_per_s_wall": n / statistics.median(wall[1:])}
    if ctx is not None:
        rec["upload_ms"] = _stats(up[1:])
        rec["insert_resolve_ms"] = _stats(ir[1:])
    return rec, last


def log_commitment(BallotBox, ctx, rng, n, reps):
    """the log-commitment figures on one path: wall medians over `reps` fresh boxes of n distinct entries"""
    pis = make_stream(rng, n + 1024 + 65536, 0)
    absent = rng.integers(0, P, size=(65536, 4), dtype=np.uint64)
    t = {k: [] for k in ("commit_from_empty", "commit_after_1024", "commit_after_65536", "find_1024", "find_65536",
                         "receipts_1024")}
    last = None
    for _ in range(reps):
        box = BallotBox(ctx, PROPOSAL, [ROOT_DIGEST], capacity=2 * n)
        box.cast_public(pis[:n], reserve=False, raw=True)

        def timed(key, fn):
            t0 = time.perf_counter()
            out = fn()
            t[key].append(time.perf_counter() - t0)
            return out
        roots = [timed("commit_from_empty", box.commit_log)]
        box.cast_public(pis[n:n + 1024], reserve=False, raw=True)
        roots.append(timed("commit_after_1024", box.commit_log))
        box.cast_public(pis[n + 1024:], reserve=False, raw=True)
        roots.append(timed("commit_after_65536", box.commit_log))
        finds, qrng = [], np.random.default_rng(3)  # the same queries in every run and on both paths
        for k in (1024, 65536):
            q = np.ascontiguousarray(pis[qrng.integers(0, n, k), 9:13])
            q[1::2] = absent[:k // 2]
            finds.append((q, timed("find_%d" % k, lambda: box.find(q, raw=True))))
        seqs = qrng.integers(0, n, 1024)
        rs = timed("receipts_1024", lambda: box.receipts(seqs))
        assert all(BallotBox.check_receipt(r) for r in rs[:8])
        last = (roots, finds, [tuple(r) for r in rs[:8]], seqs)
        box.free()
    return {k: _stats(v) for k, v in t.items()}, last


def log_audit(qp, ctx, n, reps):
    """the audit figures on one path (ctx None: the host path) for a log of n honest entries, a
    quarter of them double votes: wall medians of `reps` runs after one warm-up run"""
    BallotBox, audit_log = qp.BallotBox, qp.audit_log
    pis = make_stream(np.random.default_rng(4), n, n // 4)
    box = BallotBox(ctx, PROPOSAL, [ROOT_DIGEST], capacity=n)
    box.cast_public(pis, reserve=False, raw=True)
    entries, (root, got_n), tally = box.entries(), box.commit_log(), box.tally
    ms = [(i + 1) * n // 1024 for i in range(1024)]
    t = {}

    def timed(key, fn):
        runs = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            out = fn()
            runs.append(time.perf_counter() - t0)
            if hasattr(out, "free"):
                out.free()
        t[key] = _stats(runs[1:])
        return out
    roots = timed("roots_at_1024", lambda: box.roots_at(ms))
    box.free()
    commitments = list(zip(roots, ms))
    assert got_n == n and roots[-1] == root
    plain = timed("audit_root_tally", lambda: audit_log(ctx, entries, root=root, tally=tally))
    full = timed("audit_root_tally_1024_commitments",
                 lambda: audit_log(ctx, entries, root=root, tally=tally, commitments=commitments))
    assert plain == full and (plain.status, plain.root, (plain.yes, plain.no)) == (0, root, tally)
    timed("restore", lambda: BallotBox.restore(ctx, PROPOSAL, [ROOT_DIGEST], entries, capacity=n))
    timed("restore_root_expected", lambda: BallotBox.restore(ctx, PROPOSAL, [ROOT_DIGEST], entries, capacity=n, root=root))

    # what an auditor can do without the audit: the log's public inputs cast into a fresh box, then
    # commit_log.  It checks less: no order, no witness, no earlier commitment, and it needs the
    # ballots' public inputs, which the published log does not carry (rebuilt here from the log)
    again = np.zeros((n, 13), np.uint64)
    again[:, 0:4], again[:, 4:8] = PROPOSAL, ROOT_DIGEST
    again[:, 8], again[:, 9:13] = entries[3], entries[0]

    def recast():
        b = BallotBox(ctx, PROPOSAL, [ROOT_DIGEST], capacity=n)
        b.cast_public(again, reserve=False, raw=True)
        got = (b.commit_log()[0], b.tally)
        b.free()
        return got
    # the recast box numbers its ballots 0..n-1; the stream had no rejected ballot, so the roots agree
    assert timed("cast_public_plus_commit_log", recast) == (root, tally)
    return t, (root, tally, roots[::128], tuple(plain))


def ab_cast_child(lib_path, log_n, reps):
    """the A/B's child: cast_public, distinct, 16 batches, through plain ctypes on `lib_path`"""
    import ctypes
    L = ctypes.CDLL(lib_path)
    VP = ctypes.c_void_p
    L.qp_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(VP)]
    L.qp_ctx_destroy.argtypes = [VP]
    L.qp_ctx_destroy.restype = None
    L.qp_ballot_box_new.argtypes = [VP, VP, VP, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(VP)]
    L.qp_ballot_box_cast_public.argtypes = [VP, VP, VP, ctypes.c_uint32, VP]
    L.qp_ballot_box_tally.argtypes = [VP, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.qp_ballot_box_free.argtypes = [VP]
    L.qp_ballot_box_free.restype = None
    n = 1 << log_n
    batch = n // 16
    pis = make_stream(np.random.default_rng(1), n, 0)
    prop, root = np.array(PROPOSAL, np.uint64), np.array(ROOT_DIGEST, np.uint64)
    out = np.zeros((batch, 3), np.uint64)  # qp_ballot_result: 24 bytes
    ctx = VP()
    assert L.qp_ctx_create(0, ctypes.byref(ctx)) == 0
    wall, tally = [], None
    for _ in range(reps + 1):  # the first run is the warm-up
        box = VP()
        assert L.qp_ballot_box_new(ctx, prop.ctypes.data, root.ctypes.data, 1, 2 * n, ctypes.byref(box)) == 0
        t0 = time.perf_counter()
        for at in range(0, n, batch):
            assert L.qp_ballot_box_cast_public(box, pis[at:at + batch].ctypes.data, None, batch, out.ctypes.data) == 0
        wall.append(time.perf_counter() - t0)
        y, no = ctypes.c_uint64(), ctypes.c_uint64()
        L.qp_ballot_box_tally(box, ctypes.byref(y), ctypes.byref(no))
        tally = [y.value, no.value]
        L.qp_ballot_box_free(box)
    L.qp_ctx_destroy(ctx)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from libhash import lib_sha16
    print(json.dumps({"lib_sha16": lib_sha16(lib_path), "wall_s": _stats(wall[1:]), "runs_s": wall[1:], "tally": tally}))


def audit_records(qp, ctx, args, sha):
    """audit_log, restore and roots_at: the device at 2^log_n entries; the device and the host path
    of the same library side by side at 2^audit_host_log_n (the host path hashes 2 n permutations
    on one thread, 6 s per 2^20-leaf root: its figures are taken at the smaller size, labelled scaled)"""
    n, hn = 1 << args.log_n, 1 << args.audit_host_log_n
    dev, dlast = log_audit(qp, ctx, n, args.reps)
    sdev, slast = log_audit(qp, ctx, hn, args.reps)
    host, hlast = log_audit(qp, None, hn, args.reps)  # at the scaled size the host path affords every run
    assert slast == hlast, "device and host audits disagree"
    return {"lib_sha16": sha, "entries": n, "doubles": n // 4, "scaled_entries": hn, "log_root": dlast[0],
            "results_equal_at_scaled": True,
            "what": "wall of one call each, median of `runs` runs after one warm-up run, the same count on the device "
                    "and on the host path; the log and the claims are host arrays, so "
                    "audit_log and restore include the log's upload; roots_at: 1024 sizes spread over the log, on a "
                    "committed box; cast_public_plus_commit_log: what an auditor could do before (it checks less); "
                    "*_scaled: the same at scaled_entries, where the host path (ctx None) is run; reported, not gated",
            "device": dev, "device_scaled": sdev, "host_scaled": host,
            "device_wall_over_host_wall_scaled": {k: sdev[k]["median"] / host[k]["median"] for k in sdev}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--audit-only", action="store_true", help="only the log audit's records, into --out's log_audit key")
    ap.add_argument("--audit-host-log-n", type=int, default=16, help="log2 of the size the host path's audit runs at")
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--proofs", type=int, default=1024, help="real voting proofs of the cast / verify_batch pair (0 = skip)")
    ap.add_argument("--parent-lib", help="the parent commit's libqpgpu.so: A/B of cast_public, distinct, 16 batches")
    ap.add_argument("--ab-cast-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ballot_bench.json"))
    args = ap.parse_args()
    if args.ab_cast_child:
        return ab_cast_child(args.ab_cast_child, args.log_n, args.reps)

    import qp_wormhole
    from qp_wormhole import BallotBox
    from qp_wormhole._native import LIB_PATH
    from libhash import lib_sha16

    n = 1 << args.log_n
    cap = 2 * n
    rng = np.random.default_rng(1)
    ctx = qp_wormhole.Context(0)
    if args.audit_only:
        # the log audit's records alone, into the file's "log_audit" key; the other records stay as they are
        with open(args.out) as f:
            out = json.load(f)
        out["log_audit"] = audit_records(qp_wormhole, ctx, args, lib_sha16(LIB_PATH))
        ctx.close()
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out["log_audit"]))
        return
    out = {"lib_sha16": lib_sha16(LIB_PATH), "ballots": n, "capacity": cap, "reps": args.reps,
           "what": "wall: perf_counter around the cast_public calls of the whole stream, fresh box per run, one warm-up "
                   "run dropped; *_ms: HIP events summed over the stream's calls; host: the same library with ctx None",
           "streams": []}
    for name, doubles in (("distinct", 0), ("quarter_doubles", n // 4)):
        pis = make_stream(rng, n, doubles)
        rows = []
        for batch in (1024, 65536, n):
            dev, dlast = cast_stream(BallotBox, ctx, pis, cap, batch, args.reps)
            host, hlast = cast_stream(BallotBox, None, pis, cap, batch, args.reps)
            same = bool((dlast[0] == hlast[0]).all()) and dlast[1:] == hlast[1:]
            assert same, "device and host paths disagree"
            rows.append({"batch": batch, "device": dev, "host": host, "results_equal": same,
                         "device_wall_over_host_wall": dev["wall_s"]["median"] / host["wall_s"]["median"]})
        out["streams"].append({"name": name, "doubles": doubles, "tally": list(dlast[1]), "batches": rows})

    # reserve 2 N -> 4 N and recount on a box holding the N-ballot distinct stream
    pis = make_stream(rng, n, 0)
    for label, c in (("device", ctx), ("host", None)):
        rs, rc = [], []
        for _ in range(args.reps):
            box = BallotBox(c, PROPOSAL, [ROOT_DIGEST], capacity=cap)
            box.cast_public(pis, reserve=False, raw=True)
            t0 = time.perf_counter()
            box.reserve(2 * cap)
            rs.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            got = box.recount()
            rc.append(time.perf_counter() - t0)
            assert got[:2] == box.tally and got[2:] == (n, n)
            box.free()
        out["reserve_" + label] = {"from": cap, "to": 2 * cap, "admitted": n, "wall_s": _stats(rs)}
        out["recount_" + label] = {"admitted": n, "wall_s": _stats(rc)}

    out["real_proofs"] = "not measured"
    if args.proofs:
        from qp_wormhole import VoterRegistry, WormholeVerifier
        from qp_wormhole.prover import _verifier_only
        k = args.proofs
        keys = rng.integers(0, P, size=(k, 4), dtype=np.uint64)
        circ = qp_wormhole.Circuit.voting()
        prover = qp_wormhole.Prover(ctx, circ, k)
        reg = VoterRegistry(ctx, keys)
        proofs = reg.prove(prover, range(k), PROPOSAL, [bool(i & 1) for i in range(k)])
        ver = WormholeVerifier(circuit_data=(_verifier_only(circ, prover), circ.common_data()), max_batch=256)
        assert ver.verify_batch(proofs) == [0] * k  # warm-up
        vt, ct = {"device": [], "host": []}, {"device": [], "host": []}
        for _ in range(args.reps):
            for label, c in (("device", ctx), ("host", None)):
                t0 = time.perf_counter()
                ver.verify_batch(proofs)
                vt[label].append(time.perf_counter() - t0)
                box = BallotBox(c, PROPOSAL, [reg.root], verifier=ver, capacity=k)
                t0 = time.perf_counter()
                res = box.cast(proofs, raw=True)
                ct[label].append(time.perf_counter() - t0)
                assert (res["status"] == 0).all() and box.tally == (k // 2, k - k // 2)
                box.free()
        out["real_proofs"] = {
            "proofs": k, "verifier": "device query rounds, max_batch 256",
            "verify_batch_wall_s": _stats(vt["device"] + vt["host"]),
            "cast_device_box_wall_s": _stats(ct["device"]), "cast_host_box_wall_s": _stats(ct["host"]),
            "box_adds_s_device": statistics.median(ct["device"]) - statistics.median(vt["device"]),
            "box_adds_s_host": statistics.median(ct["host"]) - statistics.median(vt["host"])}
        ver.close()
        reg.free()
        prover.free()
        circ.free()
    # the log commitment, device beside host (the host path hashes 2 n permutations on one thread: three runs)
    dev, dlast = log_commitment(BallotBox, ctx, np.random.default_rng(2), n, args.reps)
    host, hlast = log_commitment(BallotBox, None, np.random.default_rng(2), n, min(args.reps, 3))
    assert dlast[0] == hlast[0] and dlast[2] == hlast[2], "device and host commitments disagree"
    assert all((a[1] == b[1]).all() for a, b in zip(dlast[1], hlast[1])), "device and host find disagree"
    out["log_commitment"] = {
        "entries": n, "capacity": cap, "log_root": dlast[0][0][0], "results_equal": True,
        "what": "wall of one call each on a fresh box of `entries` distinct ballots; find: half of the queries absent; "
                "receipts: 1024 random entries, BallotReceipt objects included; host: the same library with ctx None",
        "device": dev, "host": host,
        "device_wall_over_host_wall": {k: dev[k]["median"] / host[k]["median"] for k in dev}}
    out["log_audit"] = audit_records(qp_wormhole, ctx, args, out["lib_sha16"])
    ctx.close()
    out["ab_cast_public_16x65536"] = "not measured"
    if args.parent_lib:
        # two rounds, the order swapped in the second: the process that runs first in a pair is not always the same library
        rounds = []
        for order in (("parent", "this"), ("this", "parent")):
            ab = {"order": list(order)}
            for label in order:
                path = args.parent_lib if label == "parent" else LIB_PATH
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-cast-child", path, "--log-n",
                                      str(args.log_n), "--reps", "7"], check=True, capture_output=True, text=True,
                                     timeout=600)
                ab[label] = json.loads(res.stdout.strip().splitlines()[-1])
            lo, hi = ab["parent"]["wall_s"]["min"], ab["parent"]["wall_s"]["max"]
            ab["this_median_inside_parent_range"] = bool(lo <= ab["this"]["wall_s"]["median"] <= hi)
            rounds.append(ab)
        out["ab_cast_public_16x65536"] = {
            "what": "cast_public, distinct, 16 batches, fresh process per library, 7 runs after one warm-up", "rounds": rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
