"""bench.py --dump-outputs: the files dump_outputs writes for a batch of proofs
(no GPU: the proofs here are made-up byte strings)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("qp_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _proofs(n, size, short=()):
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, size - (3 if i in short else 0), dtype=np.uint8).tobytes() for i in range(n)]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_batch_is_written_whole(tmp_path):
    proofs = _proofs(5, 1000, short={2})
    _bench().dump_outputs(str(tmp_path / "out"), proofs)  # creates the directory
    a = _load(tmp_path / "out")
    assert sorted(a) == ["proof_index", "proof_lengths", "proofs"]
    assert a["proofs"].dtype == np.float32 and a["proofs"].shape == (5, 1000)
    assert a["proof_index"].dtype == np.float64 and a["proof_index"].tolist() == [0, 1, 2, 3, 4]
    assert a["proof_lengths"].dtype == np.float64 and a["proof_lengths"].tolist() == [1000, 1000, 997, 1000, 1000]
    for i, p in enumerate(proofs):
        assert a["proofs"][i, :len(p)].astype(np.uint8).tobytes() == p
        assert not a["proofs"][i, len(p):].any()


def test_no_timed_step_is_refused_by_the_parser(tmp_path, monkeypatch, capsys):
    bench = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0", "--dump-outputs", str(tmp_path / "out")])
    try:
        bench.parse()
        code = None
    except SystemExit as e:
        code = e.code
    assert code == 2 and "--steps must be at least 1" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_large_batch_is_a_fixed_sample_within_the_budget(tmp_path):
    bench = _bench()
    size = 150_000
    proofs = _proofs(4, size) * 64  # 256 proofs, 38 MB of bytes: 154 MB as float32
    bench.dump_outputs(str(tmp_path / "a"), proofs)
    bench.dump_outputs(str(tmp_path / "b"), proofs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    on_disk = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert on_disk <= 64 * 1000 * 1000
    k = len(a["proof_index"])
    assert k == (bench.DUMP_BYTES - 2 * 8 * 256 - 3 * 128) // (4 * size) and 90 <= k < 256
    idx = a["proof_index"].astype(int)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < 256
    assert a["proofs"].shape == (k, size) and len(a["proof_lengths"]) == 256
    for r in (0, k // 2, k - 1):
        assert a["proofs"][r].astype(np.uint8).tobytes() == proofs[idx[r]]
    for name in a:  # the same sample and bytes from run to run
        assert np.array_equal(a[name], b[name])
