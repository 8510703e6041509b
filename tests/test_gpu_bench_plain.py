"""A plain `bench.py` run (no --full) at a small batch: the headline line, none
of the records that take runs of their own, and --dump-outputs: the proofs of
the last timed step, which verify under the oracle verifier and are the bytes
the library gives for the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "valu_kernels", "latency_1proof_ms", "zk_config", "aggregation", "configs3",
             "prove_only_1prover_proofs_per_s", "warmup_proof_verified", "reference_proof_bytes_equal",
             "reference_bench_shapes", "dominant_kernel", "gpu_busy_frac", "profile_build", "cpu_baseline")


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "5", "--provers", "2",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=110, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["metric"] == "Wormhole proofs/sec (whole node)" and rec["unit"] == "proofs/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u64 (Goldilocks field)"
    assert rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(5 / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in rec]

    proofs = np.load(out / "proofs.npy")
    assert sorted(os.listdir(out)) == ["proof_index.npy", "proof_lengths.npy", "proofs.npy"]
    assert proofs.dtype == np.float32 and proofs.shape == (5, rec["proof_bytes"])
    assert np.load(out / "proof_index.npy").tolist() == [0, 1, 2, 3, 4]
    assert np.load(out / "proof_lengths.npy").tolist() == [rec["proof_bytes"]] * 5

    import qp_wormhole
    from oracle_lib import lib as olib
    from qp_wormhole.synthetic import synthetic_inputs
    ctx = qp_wormhole.Context(0)
    circ = qp_wormhole.Circuit.wormhole(zero_knowledge=False)
    prover = qp_wormhole.Prover(ctx, circ, max_batch=5)
    mine = prover.prove_inputs([synthetic_inputs(i) for i in range(5)])
    vd = prover.verifier_data()
    prover.free()
    ctx.close()
    for i in range(5):
        dumped = proofs[i].astype(np.uint8).tobytes()
        assert olib().ora_verify(vd, len(vd), dumped, len(dumped)) == 0
        assert dumped == mine[i]
