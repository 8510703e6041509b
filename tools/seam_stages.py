"""The three polynomial stages of INTEGRATION.md binding A that used to stay on
the host -- wires_permutation_partial_products_and_zs, OpeningSet::new and the
initial FRI polynomial -- timed two ways inside a proof composed from the seams
(tests/seam_stage_prover.py): through the seams (qp_partial_products_and_zs,
qp_opening_set, qp_fri_initial_poly: upload, kernels, copy back) and through
the host stand-ins of tests/seam_prover.py (the CPU oracle's C on this machine's
threads: NOT plonky2's times).  Beside them the whole-circuit prover's
qp_prover_stage_times slots 1, 3 and 4 for one proof of the same circuit (slot 1
also holds the Zs commitment, slot 4 every FRI reduction layer).  Circuits: the
Wormhole leaf (2^13) and the degree-2^15 aggregation of five leaf proofs.
Host clock around calls that end synchronised; median of --runs after a warm-up.

  python tools/seam_stages.py [--runs 7] [--out profiles/seam_stages.json]

Every GPU step (one circuit each) runs as a child process under its own time
limit; a step that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "qp-zk-circuits-rm_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

STEPS = {"wormhole": 240, "aggregation_2^15": 420}  # seconds allowed per GPU step
SEAM_STAGES = ("zs", "openings", "fri_initial")
PROVER_SLOTS = {"zs": "zs_pp", "openings": "openings", "fri_initial": "fri"}  # qp_prover_stage_times 1, 3, 4


def make_circuit(name):
    import qp_wormhole
    if name == "wormhole":
        import wormhole_inputs as WI
        circ = qp_wormhole.Circuit.wormhole()
        return circ, circ.commit(WI.test_inputs())
    from current_circuit_vd import current_circuit_verifier_data
    from oracle_lib import golden
    from test_oracle_golden import current_common_bytes
    cb = current_common_bytes()
    vd = current_circuit_verifier_data(cb)[0]
    leaves = [golden("dummy_proof.bin"), golden("dummy_proof_zk.bin")]
    circ = qp_wormhole.Circuit.aggregation(cb, 5)
    return circ, circ.commit_proofs(vd[:len(vd) - len(cb)], [leaves[i % 2] for i in range(5)])


def step(name, runs):
    """one circuit: prove through the seams, through the host stand-ins, and with the whole-circuit prover"""
    import qp_wormhole
    from seam_stage_prover import prove
    ctx = qp_wormhole.Context(0)
    circ, w = make_circuit(name)
    wires, pis = w.wires(), w.public_inputs()
    g = qp_wormhole.gate_desc(circ)
    res = {"degree_bits": circ.degree_bits, "num_routed_wires": g.num_routed_wires, "num_wires": g.num_wires,
           "runs": runs}
    proofs = {}
    for mode in ("seam", "host"):
        proofs[mode] = prove(ctx, circ, wires, pis, stages=mode)  # warm-up
        times = {}
        for _ in range(runs):
            assert prove(ctx, circ, wires, pis, stages=mode, times=times) == proofs[mode]
        res["seam_ms" if mode == "seam" else "host_stand_in_oracle_c_ms"] = {
            k: statistics.median(times[k]) * 1e3 for k in SEAM_STAGES}
    whole = qp_wormhole.Prover(ctx, circ, 1)
    ref = whole.prove_witnesses([w])[0]  # warm-up
    assert proofs["seam"] == ref and proofs["host"] == ref
    per = {k: [] for k in SEAM_STAGES}
    for _ in range(runs):
        whole.stage_times(reset=True)
        whole.prove_witnesses([w])
        st = whole.stage_times()
        for k in SEAM_STAGES:
            per[k].append(st[PROVER_SLOTS[k]])
    res["whole_circuit_prover_stage_ms"] = {k: statistics.median(per[k]) for k in SEAM_STAGES}
    whole.free()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_stages.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="(internal) run one GPU step and print its JSON")
    a = ap.parse_args()
    if a.runs < 5:
        ap.error("--runs must be at least 5")
    if a.step:
        print("SEAM_STAGES_STEP " + json.dumps(step(a.step, a.runs)))
        return
    from libhash import lib_sha16
    res = {"command": "python tools/seam_stages.py --runs %d" % a.runs, "lib_sha16": lib_sha16(),
           "host_threads": min(os.cpu_count() or 4, 16),
           "note": "median ms per stage inside one composed proof; host stand-ins are the CPU oracle's C "
                   "(tests/seam_prover.py), not plonky2; whole-circuit slot zs also commits the Zs, slot "
                   "fri_initial (qp_prover_stage_times[4]) also runs every FRI reduction layer",
           "circuits": {}}
    for name, limit in STEPS.items():
        # a fresh child per step: its own time limit, and a failure starts nothing further on the device
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--runs", str(a.runs)],
                           stdout=subprocess.PIPE, text=True, timeout=limit)
        if p.returncode:
            sys.exit("step %s failed with status %d" % (name, p.returncode))
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("SEAM_STAGES_STEP ")][-1]
        res["circuits"][name] = json.loads(line[len("SEAM_STAGES_STEP "):])
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
