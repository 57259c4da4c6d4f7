"""bench.py's own surface: the plain run and --full, and the arrays --dump-outputs writes (their layout on host tensors here; on the
device, -m gpu, against numpy's QR of the same seeded input)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    env = dict(os.environ)                   # bench.py sets an HSA variable at import: keep it out of this process
    try:
        spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        os.environ.clear()
        os.environ.update(env)
    return mod


def test_bench_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out.stdout


def _column_major(m, n, seed):
    """A torch image of an m x n column-major matrix, as bench.py's buffers are: shape (n, m), row c = column c."""
    import torch
    M = np.random.default_rng(seed).random((m, n))
    return M, torch.from_numpy(np.ascontiguousarray(M.T))


def test_dump_outputs_whole_arrays_when_small(tmp_path):
    b = _bench_module()
    m, n = 40, 8
    A, At = _column_major(m, n, 1)
    R, Rt = _column_major(n, n, 2)
    names = b.dump_outputs(str(tmp_path), At, Rt, m, n)
    assert names == ["R_diag", "R_last_column", "R_sample", "factors_sample"]
    got = {k: np.load(tmp_path / (k + ".npy")) for k in names}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["R_diag"], np.diag(R)) and np.array_equal(got["R_last_column"], R[:, -1])
    assert np.array_equal(got["R_sample"], np.concatenate([R[:j + 1, j] for j in range(n)]))     # upper triangle, column by column
    assert np.array_equal(got["factors_sample"], A.reshape(-1, order="F"))


def test_dump_outputs_samples_are_seeded_and_bounded(tmp_path, monkeypatch):
    b = _bench_module()
    assert 2 * b.DUMP_SAMPLE * 8 <= 48 << 20                      # the samples leave room for R_diag / R_last_column under 64 MB
    monkeypatch.setattr(b, "DUMP_SAMPLE", 500)
    m, n = 300, 120
    A, At = _column_major(m, n, 3)
    R, Rt = _column_major(n, n, 4)
    R = np.triu(R)
    Rt = Rt.tril()                                                # the transposed image of an upper-triangular R
    b.dump_outputs(str(tmp_path / "a"), At, Rt, m, n)
    b.dump_outputs(str(tmp_path / "b"), At, Rt, m, n)
    for k in ("R_sample", "factors_sample"):
        x, y = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert x.shape == (500,) and np.array_equal(x, y)
    rs = np.load(tmp_path / "a" / "R_sample.npy")
    assert np.isin(rs, R[np.triu_indices(n)]).all() and np.count_nonzero(rs) > 450    # drawn from the upper triangle only
    assert np.isin(np.load(tmp_path / "a" / "factors_sample.npy"), A).all()


def _run_bench(args, timeout=600):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + args, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_and_full_bench_lines_and_dumped_outputs(tmp_path):
    """A plain run (C2 4096^2, 3 timed steps) prints the headline fields and nothing it did not measure; --full adds roofline and accuracy;
    both dump the last timed step, which is the factorisation of the generator's seed-14 matrix (seeds 12 + i, one buffer per step)."""
    import cuda_qr_amd as qr
    K, W = 3, 1
    plain = _run_bench(["--workload", "c2", "--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == K and plain["warmup"] == W and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["unit"] == "GFLOP/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64" and plain["full"] is False
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["accuracy"] == {}
    full = _run_bench(["--workload", "c2", "--steps", str(K), "--warmup", str(W), "--full", "--no-cpu-baseline",
                       "--dump-outputs", str(tmp_path / "full")])
    assert full["full"] is True and full["roofline"]["achieved"] > 0 and full["accuracy"]["resid"] < 1e-13
    n = 4096
    A = qr.uniform_matrix_host(n, n, seed=12 + W + K - 1)
    Rn = np.linalg.qr(A, mode="r")
    s = np.sign(np.diag(Rn))
    total = 0
    for name in ("plain", "full"):
        d = {k: np.load(tmp_path / name / (k + ".npy")) for k in ("R_diag", "R_last_column", "R_sample", "factors_sample")}
        total = max(total, sum(v.nbytes for v in d.values()))
        sd = np.sign(d["R_diag"])
        assert np.linalg.norm(sd * d["R_diag"] - s * np.diag(Rn)) / np.linalg.norm(np.diag(Rn)) < 1e-12
        assert np.linalg.norm(sd * d["R_last_column"] - s * Rn[:, -1]) / np.linalg.norm(Rn[:, -1]) < 1e-12
    assert total <= 64 << 20
    for k in ("R_diag", "R_last_column", "R_sample", "factors_sample"):      # same arguments, same input: the same results
        x, y = np.load(tmp_path / "plain" / (k + ".npy")), np.load(tmp_path / "full" / (k + ".npy"))
        assert np.allclose(x, y, rtol=0, atol=1e-12 * np.abs(x).max())
