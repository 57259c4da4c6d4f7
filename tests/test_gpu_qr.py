"""-m gpu: parity of the HIP path (through the C-ABI) with the reference qr.c.

Parity definition (fp64): with S = diag(sign(diag R)),
    ||S R_hip - S' R_ref||_F / ||R_ref||_F <= 1e-13      (R_ref from golden fixtures made by the REAL reference)
    ||A - Q R||_F / ||A||_F < 1e-12   (north-star tolerance; observed ~1e-15)
    ||Q^T Q - I||_F <= 1e-12 * sqrt(n)-scale (the reference itself gives 3.5e-14 .. 9.4e-14 at C1)
V / tau are NOT compared: their layout depends on the reference's compile-time window (qr.c:12-13,300-304).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import dev, host, rel, zeros

pytestmark = pytest.mark.gpu

GOLD = [("ref_6x4_f64_4x2", 6, 4), ("ref_128x32_f64_4x2", 128, 32), ("ref_120x32_f64_64x8", 120, 32),
        ("ref_64x20_f64_16x4", 64, 20), ("ref_512x128_f64_64x8", 512, 128), ("ref_512x128_f64_4x2", 512, 128)]


def golden_R(g, n):
    if "Rn" in g:
        return g["Rn"]
    R = np.zeros((n, n))
    R[np.triu_indices(n)] = g["Rn_triu"]
    return R


@pytest.mark.parametrize("name,m,n", GOLD)
def test_dropin_mmqr_explicitQR_vs_reference_golden(qr, oracle, name, m, n):
    """mmqr + explicitQR through the drop-in host-pointer ABI on the reference's own input
    (srand(12)/rand(), qr.c:468-474) against outputs of the real reference."""
    g = load_golden(name)
    A = oracle.fill_rand(m, n)
    F, tau = qr.mmqr(A)
    rp, cp = qr.get_panel_dims(m, n)
    assert tau.shape[0] == rp * cp * qr.default_block_size(m, n)[0] >= n        # qr.c:61 sizing rule
    Rn = oracle.sign_normalise(F)
    assert rel(Rn, golden_R(g, n)) <= 1e-13
    assert np.abs(np.abs(np.diag(F[:n])) - np.abs(g["diagR"])).max() < 1e-12 * np.abs(g["diagR"]).max()
    Q, R = qr.explicit_qr(F, tau)
    assert Q.shape == (m, m) and R.shape == (m, n)
    assert np.array_equal(R, np.triu(F)), "R must be the upper triangle of the factored matrix (qr.c:334-343)"
    resid = np.linalg.norm(A - Q @ R) / np.linalg.norm(A)
    orth = np.linalg.norm(Q.T @ Q - np.eye(m))
    assert resid < 1e-12 and orth < 1e-12 * np.sqrt(m) * 4
    if "resid" in g:      # not worse than an order of magnitude over the reference's own accuracy
        assert resid < 10 * max(float(g["resid"]), 1e-15) and orth < 10 * max(float(g["orth"]), 1e-14)
    # Q's leading n columns agree with the reference's up to the same row signs as R
    if "Q" in g:
        s = np.sign(np.diag(F[:n])) * np.sign(g["diagR"])
        assert np.abs(Q[:, :n] * s[None, :] - g["Q"][:, :n]).max() < 1e-12


@pytest.mark.parametrize("name,m,n", [("ref_6x4_f32_4x2", 6, 4)])
def test_float_instantiation_vs_reference_float_golden(qr, oracle, name, m, n):
    """The reference as committed is a float program (qr.c:11).  mmqr_f32 / explicitQR_f32 on its own 6 x 4 float self-test input
    against the outputs of the real float reference: sign-normalised R to float round-off, and a residual no worse than the
    3.8e-07 the reference prints (qr.c:505-515)."""
    g = load_golden(name)
    A = oracle.fill_rand(m, n, 12, np.float32)
    assert np.array_equal(A, g["A"])
    F, tau = qr.mmqr_f32(A)
    assert F.dtype == np.float32 and tau.dtype == np.float32
    Rn = oracle.sign_normalise(F.astype(np.float64))
    assert rel(Rn, g["Rn"].astype(np.float64)) < 5e-7
    Q, R = qr.explicit_qr_f32(F, tau)
    A64, Q64, R64 = A.astype(np.float64), Q.astype(np.float64), R.astype(np.float64)
    assert np.sqrt(((Q64 @ R64 - A64) ** 2).sum()) < 3.8e-07 * 2
    assert np.linalg.norm(Q64.T @ Q64 - np.eye(m)) < 1e-6
    # a bigger float case: accuracy of a float caller is bounded by the storage precision only
    B = np.random.default_rng(5).random((700, 130)).astype(np.float32)
    Fb, taub = qr.mmqr_f32(B)
    Qb, Rb = qr.explicit_qr_f32(Fb, taub)
    B64 = B.astype(np.float64)
    assert np.linalg.norm(Qb.astype(np.float64) @ Rb.astype(np.float64) - B64) / np.linalg.norm(B64) < 5e-7


def test_reference_self_check_flow(qr, oracle):
    """The reference's main() (qr.c:461-515): 6x4, mmqr, explicitQR, dgemm(Q,R), unnormalised residual."""
    A = oracle.fill_rand(6, 4)
    F, tau = qr.mmqr(A)
    Q, R = qr.explicit_qr(F, tau)
    QR = qr.dgemm(Q, R)
    assert np.sqrt(((QR - A) ** 2).sum()) < 1e-14          # reference prints 3.8e-07 in float, 7e-16 in double


@pytest.mark.parametrize("k,m,n", [(6, 6, 4), (37, 91, 13), (512, 512, 128), (300, 5, 700)])
def test_dropin_dgemm(qr, k, m, n):
    rng = np.random.default_rng(k + m + n)
    A, B = rng.standard_normal((k, m)), rng.standard_normal((m, n))
    assert rel(qr.dgemm(A, B), A @ B) < 1e-14


SHAPES = [(1, 1), (2, 2), (7, 3), (33, 33), (100, 64), (129, 128), (257, 130), (640, 384), (1000, 1000),
          (2048, 96), (5000, 33), (300, 300)]


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("nb,ib", [(128, 32), (32, 8), (512, 32)])
def test_geqrf_applyq_ragged_shapes(qr, oracle, m, n, nb, ib):
    """Edge cases the reference cannot even run (it needs (m-PR)%(PR-PC)==0, n%PC==0): any m >= n."""
    rng = np.random.default_rng(m * 31 + n)
    A = rng.standard_normal((m, n))
    p = qr.Plan(m, n, nb, ib)
    dA, dtau, dQ, dR = dev(A), zeros(n, 1), zeros(m, n), zeros(n, n)
    torch.cuda.synchronize()
    p.geqrf(dA, m, n, m, dtau)
    p.extract_r(dA, m, n, m, dR, n, n)
    p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
    p.sync()
    R, Q = host(dR), host(dQ)
    assert np.array_equal(np.tril(R, -1), np.zeros((n, n)))
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(R), ref) < 1e-12
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-13 * max(8, n)
    p.close()


def test_geqrf_with_lda_and_submatrix(qr, oracle):
    rng = np.random.default_rng(2)
    m, n, lda = 300, 70, 410
    buf = rng.standard_normal((lda, n + 5))
    dA = dev(buf)
    p = qr.Plan(m, n, 64, 16)
    dtau = zeros(n, 1)
    torch.cuda.synchronize()
    sub = dA.data_ptr() + 8 * (2 * lda + 10)                # start at row 10, column 2
    p.geqrf(sub, m, n, lda, dtau)
    p.sync()
    out = host(dA)
    mask = np.ones_like(buf, dtype=bool)
    mask[10:10 + m, 2:2 + n] = False
    assert np.array_equal(out[mask], buf[mask]), "nothing outside the m x n window may change"
    R = oracle.sign_normalise(out[10:10 + m, 2:2 + n])
    assert rel(R, oracle.sign_normalise(np.linalg.qr(buf[10:10 + m, 2:2 + n], mode="r"))) < 1e-12
    p.close()


def test_rank_deficient_and_zero_columns(qr):
    """The reference returns NaN for a zero column (qr.c:152); this build follows dlarfg (tau = 0)."""
    rng = np.random.default_rng(4)
    A = rng.standard_normal((200, 40))
    A[:, 7] = 0.0
    A[:, 20] = A[:, 3]                                      # exact dependency
    F, tau = qr.mmqr(A)
    assert np.isfinite(F).all() and np.isfinite(tau).all()
    Q, R = qr.explicit_qr(F, tau)
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(200)) < 1e-12


@pytest.mark.parametrize("m,n,cond", [(3000, 200, 1e8), (3000, 200, 1e14), (700, 130, 1e12), (20000, 64, 1e13)])
def test_ill_conditioned_matrices_stay_backward_stable(qr, m, n, cond):
    """Householder QR is backward stable whatever the conditioning: ||A - QR||/||A|| and ||Q^T Q - I|| stay at
    round-off for graded singular values up to 1e14 (this is what rules out Gram/Cholesky-type shortcuts in the
    panel and what the TSQR + Householder-reconstruction leaf has to preserve)."""
    rng = np.random.default_rng(int(np.log10(cond)) + m)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    sv = np.logspace(0, -np.log10(cond), n)
    A = (U * sv) @ V.T
    A[:, n // 2] = A[:, 3] * (1 + 1e-13) + 1e-15 * rng.standard_normal(m)       # an almost exactly repeated column
    Q, R = qr.qr_thin(A, nb=128, nshards=1)
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 5e-15 * np.sqrt(n)
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-13 * n
    # column scaling by 1e+-150 must not overflow/underflow into garbage (no dlarfg rescaling needed at these scales)
    D = np.logspace(-100, 100, n)
    Q2, R2 = qr.qr_thin(A * D, nb=128, nshards=1)
    assert np.isfinite(R2).all()
    assert np.linalg.norm(Q2.T @ Q2 - np.eye(n)) < 1e-13 * n


@pytest.mark.parametrize("m,n,P", [(1024, 64, 1), (1024, 64, 2), (1024, 64, 4), (4096, 256, 8), (999, 40, 3)])
def test_qr_thin_tsqr_shard_invariance(qr, oracle, m, n, P):
    """TSQR over P row shards on one device (SURVEY 8e 'test without 8 GPUs'): R is shard-count
    invariant after sign normalisation to 1e-13; Q is orthonormal and reproduces A."""
    A = qr.uniform_matrix_host(m, n, seed=12)
    Q, R = qr.qr_thin(A, nb=32 if n < 128 else 128, nshards=P)
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(R), ref) < 1e-13
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-13 * n


@pytest.mark.parametrize("m,n", [(1541, 1100), (777, 555), (5001, 300), (2050, 2049)])
def test_host_pointer_entry_points_pad_odd_heights(qr, oracle, m, n):
    """mmqr / qr_thin on heights that are not multiples of 16: factored with zero rows appended on the device (an odd height keeps every
    kernel off its aligned path: 5001^2 took three times as long as 5000^2); what comes back is the m x n factored form / the thin
    factors of the caller's matrix -- R against LAPACK, explicitQR on the returned factors, rows beyond m never touched."""
    rng = np.random.default_rng(m + n)
    A = rng.random((m, n))
    F, tau = qr.mmqr(A)
    assert F.shape == (m, n) and tau.shape[0] == qr.tau_len(m, n) >= n
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(F), ref) < 1e-13
    if m <= 2100:
        Q, R = qr.explicit_qr(F, tau)                       # the factors are an ordinary compact-WY form of the UNPADDED matrix
        assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-13
        assert np.linalg.norm(Q.T @ Q - np.eye(m)) < 1e-12
    Qt, Rt = qr.qr_thin(A, nb=128, nshards=1)
    assert Qt.shape == (m, n)
    assert rel(oracle.sign_normalise(Rt), ref) < 1e-13
    assert np.linalg.norm(A - Qt @ Rt) / np.linalg.norm(A) < 1e-13 and np.linalg.norm(Qt.T @ Qt - np.eye(n)) < 1e-13 * n


@pytest.mark.parametrize("m,n", [(4096, 256), (999, 40)])
def test_qr_thin_mgpu_single_device_matches_qr_thin(qr, oracle, m, n):
    """C-level TSQR entry with ngpu = 1 (no communicator): same factors as qr_thin; ngpu beyond the visible devices is refused."""
    A = qr.uniform_matrix_host(m, n, seed=12)
    Q1, R1 = qr.qr_thin(A, nb=32 if n < 128 else 128, nshards=1)
    Qg, Rg = qr.qr_thin_mgpu(A, nb=32 if n < 128 else 128, ngpu=1)
    assert rel(oracle.sign_normalise(Rg), oracle.sign_normalise(R1)) < 1e-13
    assert rel(Qg @ Rg, A) < 1e-13 and np.abs(Qg.T @ Qg - np.eye(n)).max() < 1e-12
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.qr_thin_mgpu(A, ngpu=torch.cuda.device_count() + 1)


def test_qr_thin_mgpu_all_visible_devices(qr, oracle):
    """One host thread per GPU + one RCCL all-gather, on every device of the node (skipped on a 1-GPU box)."""
    P = torch.cuda.device_count()
    if P < 2:
        pytest.skip("needs at least 2 GPUs")
    m, n = 65536, 256
    A = qr.uniform_matrix_host(m, n, seed=12)
    Q1, R1 = qr.qr_thin(A, nb=128, nshards=1)
    Qg, Rg = qr.qr_thin_mgpu(A, nb=128, ngpu=P)
    assert rel(oracle.sign_normalise(Rg), oracle.sign_normalise(R1)) < 1e-13
    assert rel(Qg @ Rg, A) < 1e-13 and np.abs(Qg.T @ Qg - np.eye(n)).max() < 1e-12


def test_dropin_mmqr_reuses_its_plan(qr, oracle):
    """Repeated host-pointer calls on same-sized matrices (the reference harness: qr.cu:776-789) run on a cached plan: the
    second and third call must not pay plan creation again, and results stay identical."""
    import time
    A = oracle.fill_rand(1024, 64)
    qr.release_cached_plans()
    outs, times = [], []
    for _ in range(4):
        t0 = time.perf_counter()
        F, tau = qr.mmqr(A)
        times.append(time.perf_counter() - t0)
        outs.append((F, tau))
    for F, tau in outs[1:]:
        assert np.array_equal(F, outs[0][0]) and np.array_equal(tau, outs[0][1])
    assert min(times[1:]) < 2e-3, times                 # < 2 ms per call once the plan exists (was ~10 ms every call)
    qr.release_cached_plans()
    F2, _ = qr.mmqr(A)
    assert np.array_equal(F2, outs[0][0])


def _device_metrics(qr, p, dA, m, n, seed):
    """||A - QR||_F/||A||_F and ||Q^T Q - I||_F computed on the device for sizes numpy would crawl on."""
    dtau, dQ, dR = zeros(n, 1), zeros(m, n), zeros(n, n)
    torch.cuda.synchronize()
    p.geqrf(dA, m, n, m, dtau)
    p.extract_r(dA, m, n, m, dR, n, n)
    p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
    dQR, dG = zeros(m, n), zeros(n, n)
    p.gemm("N", m, n, n, 1.0, dQ, m, dR, n, 0.0, dQR, m)
    p.gemm("T", n, n, m, 1.0, dQ, m, dQ, m, 0.0, dG, n)
    p.sync()
    d, a = p.diffnorm(dQR, m, m, n, seed=seed)            # A regenerated from the hash
    o, _ = p.diffnorm(dG, n, n, n, mode=1)
    return np.sqrt(d / a), np.sqrt(o), dR


def test_c2_4096_square_nb64_properties(qr):
    """BASELINE config C2: 4096 x 4096, block size 64 -- size-independent properties at full size."""
    m = n = 4096
    p = qr.Plan(m, n, 64, 32)
    dA = zeros(m, n)
    p.fill_uniform(dA, m, m, n, seed=12)
    p.sync()
    resid, orth, dR = _device_metrics(qr, p, dA, m, n, 12)
    assert resid < 1e-12 and orth < 1e-11
    # the FULL sign-normalised R against LAPACK on the same matrix (host copy of the generator): the parity definition of the
    # small golden cases, at the configuration's own size
    A = qr.uniform_matrix_host(m, n, seed=12)
    Rl = np.linalg.qr(A, mode="r")
    Rl = np.triu(Rl) * np.where(np.diag(Rl) < 0, -1.0, 1.0)[:, None]
    R = host(dR)
    assert np.array_equal(np.tril(R, -1), np.zeros_like(R))
    Rn = R * np.where(np.diag(R) < 0, -1.0, 1.0)[:, None]
    assert rel(Rn, Rl) < 1e-12                                              # observed ~1e-15
    assert np.abs(np.diag(Rn) - np.diag(Rl)).max() < 1e-12 * np.abs(np.diag(Rl)).max()
    p.close()


@pytest.mark.parametrize("nb", [32, 64, 128, 256, 512])
def test_c3_16384_square_properties(qr, nb):
    """BASELINE config C3 at full size (16384 x 16384) over its block-size sweep 32/64/128/256: residual < 1e-12
    (north-star), orthogonality.
    Also the regression test for the look-ahead race fixed in round 1 (panel and wide update sharing
    one W buffer only went wrong once the wide GEMM outlasted the next panel, i.e. at this size)."""
    m = n = 16384
    p = qr.Plan(m, n, nb, 32)
    dA = zeros(m, n)
    p.fill_uniform(dA, m, m, n, seed=12)
    p.sync()
    resid, orth, dR = _device_metrics(qr, p, dA, m, n, 12)
    assert resid < 5e-14 and orth < 1e-11          # observed 5.3e-15 / 1.0e-12 at nb = 256
    # R itself against LAPACK dgeqrf of the same matrix: slices of the sign-normalised factor computed once on the CPU
    # (oracle/make_lapack_slices.py -> tests/golden/lapack_16384_slices.npz: diagonal, row norms, three blocks, the last column)
    g = load_golden("lapack_16384_slices")
    assert int(g["n"]) == n and int(g["seed"]) == 12
    R = host(dR)
    sgn = np.where(np.diag(R) < 0, -1.0, 1.0)
    h = n // 2
    assert np.abs(np.abs(np.diag(R)) - g["diag"]).max() < 1e-12 * g["diag"].max()
    rn = np.sqrt((R * R).sum(axis=1))
    assert np.abs(rn - g["rownorm"]).max() < 1e-12 * g["rownorm"].max()
    for got, ref in ((sgn[:32, None] * R[:32, n - 256:], g["top_right"]),
                     (sgn[h:h + 48, None] * R[h:h + 48, h:h + 512], g["middle"]),
                     (sgn[n - 128:, None] * R[n - 128:, n - 128:], g["bottom_right"]),
                     (sgn * R[:, n - 1], g["col_last"])):
        assert rel(got, ref) < 1e-12                                        # observed ~1e-14
    p.close()


def test_lookahead_matches_sequential_schedule(qr, oracle, tmp_path):
    """Same matrix through the two-stream look-ahead schedule and the single-stream schedule."""
    import subprocess, sys, os, json
    code = ("import sys, json, numpy as np, torch; sys.path.insert(0, %r); import cuda_qr_amd as q;"
            "m,n=6144,3072; p=q.Plan(m,n,128,32); A=torch.empty((n,m),dtype=torch.float64,device='cuda');"
            "t=torch.empty(n,dtype=torch.float64,device='cuda'); p.fill_uniform(A,m,m,n,seed=5); p.geqrf(A,m,n,m,t); p.sync();"
            "R=np.triu(A.cpu().numpy().T[:n]); np.save(sys.argv[1], R)") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for la in ("1", "0"):
        path = str(tmp_path / f"la_{la}.npy")
        env = dict(os.environ, MI355XQR_LOOKAHEAD=la)
        subprocess.run([sys.executable, "-c", code, path], check=True, env=env)
        outs.append(np.load(path))
    assert rel(oracle.sign_normalise(outs[0]), oracle.sign_normalise(outs[1])) < 1e-13


@pytest.mark.parametrize("m,n", [(2829, 2829), (2828, 2828), (3073, 1024), (8193, 2048), (8192, 2048), (1024, 511), (8192, 512), (777, 555),
                                 (6000, 4100), (4100, 4100), (4160, 2112)])    # (the last three: ragged bottom tile / ragged width of the update kernel, half tiles)
def test_shapes_next_to_the_block_size_and_schedule_thresholds(qr, oracle, m, n):
    """The library's own choice of block size and schedule (nb = 0: qr_host.c lookahead_pays / default_blocks, measured rule of round 6) on
    shapes either side of its thresholds -- 8 M elements, m = 3 n, 8192 rows, 512 columns -- and ragged ones: sign-normalised R against
    LAPACK, residual through the device API (more shapes: devtools/tools_fuzz_parity.py 6 edges6)."""
    rng = np.random.default_rng(m * 31 + n)
    A = rng.random((m, n))
    p = qr.Plan(m, n, 0, 0)
    dA, dtau, dR = dev(A), zeros(n, 1), zeros(n, n)
    p.geqrf(dA, m, n, m, dtau); p.extract_r(dA, m, n, m, dR, n, n); p.sync()
    assert rel(oracle.sign_normalise(host(dR)), oracle.sign_normalise(np.linalg.qr(A, mode="r"))) < 1e-13
    dQ, dQR = zeros(m, n), zeros(m, n)
    p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
    p.gemm("N", m, n, n, 1.0, dQ, m, dR, n, 0.0, dQR, m); p.sync()
    assert np.linalg.norm(host(dQR) - A) / np.linalg.norm(A) < 1e-13
    p.close()


@pytest.mark.parametrize("m,n,lda,off", [(4096, 1024, 4097, 0), (4096, 1024, 4100, 1), (2049, 700, 2051, 0), (5001, 640, 5001, 0)])
def test_geqrf_dev_on_odd_leading_dimensions_and_misaligned_arrays(qr, oracle, m, n, lda, off):
    """qr_geqrf_dev on the caller's own array when its height is not a multiple of 16, its leading dimension odd or its first element not 16-byte
    aligned: the plan factors a re-pitched, zero-padded copy and copies the m rows back -- R against LAPACK, the rows between m and lda and the
    elements in front of the array never written."""
    rng = np.random.default_rng(m + n + lda)
    A = rng.random((m, n))
    buf = np.full(lda * n + off, 7.25)
    buf[off:].reshape(n, lda)[:, :m] = A.T                         # column-major with leading dimension lda, `off` doubles into the allocation
    d = torch.from_numpy(buf).cuda()
    dtau = zeros(n, 1)
    torch.cuda.synchronize()
    p = qr.Plan(m, n, 0, 0)
    p.geqrf(d[off:], m, n, lda, dtau)
    p.sync()
    out = d.cpu().numpy()
    p.close()
    assert np.array_equal(out[:off], buf[:off])
    F = out[off:].reshape(n, lda)
    assert np.array_equal(F[:, m:], np.full((n, lda - m), 7.25)), "rows beyond m are the caller's"
    R = np.triu(F[:, :m].T[:n])
    assert rel(oracle.sign_normalise(R), oracle.sign_normalise(np.linalg.qr(A, mode="r"))) < 1e-13
    assert np.all(np.isfinite(F[:, :m]))


def test_cu_split_that_is_not_a_multiple_of_32(qr, oracle, tmp_path):
    """MI355XQR_SPLIT=48: the dispatcher deals workgroups evenly over the shader engines whatever the mask says, so the one-launch panel
    (workgroups waiting for each other) may only count on whole multiples of 32 of a mask (qrd_stream_cus_coresident); before, its hand-off
    timed out on a 6144-row panel (status -105).  Same R as the single-stream schedule."""
    import subprocess, sys, os
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); import cuda_qr_amd as q;"
            "m,n=6144,2048; p=q.Plan(m,n,256,32); A=torch.empty((n,m),dtype=torch.float64,device='cuda');"
            "t=torch.empty(n,dtype=torch.float64,device='cuda'); p.fill_uniform(A,m,m,n,seed=5); p.geqrf(A,m,n,m,t); p.sync();"
            "R=np.triu(A.cpu().numpy().T[:n]); np.save(sys.argv[1], R)") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for env_add in ({"MI355XQR_LOOKAHEAD": "1", "MI355XQR_SPLIT": "48"}, {"MI355XQR_LOOKAHEAD": "0"}):
        path = str(tmp_path / ("split48_%d.npy" % len(outs)))
        subprocess.run([sys.executable, "-c", code, path], check=True, env=dict(os.environ, **env_add), timeout=300)
        outs.append(np.load(path))
    assert rel(oracle.sign_normalise(outs[0]), oracle.sign_normalise(outs[1])) < 1e-13


def test_tsqr_backend_pipelined_stack_factor(qr, oracle):
    """HipBackend.stack_factor(wait=False) leaves the stacked QR queued on its own plan while the next local QR runs
    (bench.py's pipelined TSQR steps): same R as the synchronous call."""
    from cuda_qr_amd import tsqr as T
    m, n, P = 8192, 256, 4
    be = T.HipBackend(qr, m, n, P, 128, 32)
    A = be.new_matrix(m, n); be.fill(A, m, n, 0, m, 3)
    S1 = be.new_matrix(P * n, n); S2 = be.new_matrix(P * n, n)
    be.plan.fill_uniform(S1, P * n, P * n, n, seed=9); be.plan.fill_uniform(S2, P * n, P * n, n, seed=9); be.plan.sync()
    Ra, Rb, Rl = be.new_matrix(n, n), be.new_matrix(n, n), be.new_matrix(n, n)
    be.stack_factor(S1, Ra)                                   # synchronous
    be.stack_factor(S2, Rb, wait=False)                       # queued ...
    be.local_factor(A, Rl)                                    # ... under a local factorisation on the other plan
    be.stack_sync()
    assert np.array_equal(host(Ra), host(Rb))
    Ah = qr.uniform_matrix_host(P * n, n, seed=9)
    ref = oracle.sign_normalise(np.linalg.qr(Ah, mode="r"))
    assert rel(oracle.sign_normalise(np.triu(host(Ra))), ref) < 1e-13
    be.close()


@pytest.mark.parametrize("m,n", [(262144, 256), (262144, 512)])
def test_c4_c5_full_height_properties(qr, m, n):
    """C4 at its full size on one GPU (262144 x 256) and one C5 shard (262144 x 512): residual, orthogonality of the thin
    Q, upper-triangular R with the column norms of A on... (||R||_F = ||A||_F)."""
    p = qr.Plan(m, n, 128, 32)
    dA = zeros(m, n)
    p.fill_uniform(dA, m, m, n, seed=12)
    p.sync()
    resid, orth, dR = _device_metrics(qr, p, dA, m, n, 12)
    assert resid < 1e-12 and orth < 1e-11
    R = host(dR)
    assert np.array_equal(np.tril(R, -1), np.zeros_like(R))
    # ||R||_F^2 = ||A||_F^2 = sum of squares of uniform[0,1) entries ~ m*n/3
    assert abs(np.linalg.norm(R) ** 2 / (m * n / 3.0) - 1.0) < 1e-2
    p.close()


def test_c5_full_size_single_gpu_and_8_virtual_shards(qr, oracle):
    """BASELINE config C5 at its FULL size on one GPU: 2 097 152 x 512 (8 GiB, generated in place by the counter hash -- no
    host copy), (a) factored whole (the P = 1 denominator of the 8-GPU run) with residual and orthogonality
    computed on the device, and (b) as 8 row shards of 262144 x 512 through the device API with a copy in place of the
    all-gather: R must be shard-count invariant after sign normalisation."""
    m, n, P = 2097152, 512, 8
    ms = m // P
    dA = zeros(m, n)
    p1 = qr.Plan(m, n, 128, 32)
    p1.fill_uniform(dA, m, m, n, seed=12)
    p1.sync()
    resid, orth, dR = _device_metrics(qr, p1, dA, m, n, 12)
    assert resid < 1e-12 and orth < 1e-11
    R1 = host(dR)
    assert np.array_equal(np.tril(R1, -1), np.zeros_like(R1))
    assert abs(np.linalg.norm(R1) ** 2 / (m * n / 3.0) - 1.0) < 1e-2          # ||R||_F^2 = ||A||_F^2 ~ m n / 3
    p1.close()
    # (b) 8 shards: rows [s ms, (s+1) ms) of the SAME matrix (regenerated in place), each factored with lda = m
    ps, p2 = qr.Plan(ms, n, 128, 32), qr.Plan(P * n, n, 128, 32)
    ps.fill_uniform(dA, m, m, n, seed=12)
    ps.sync()
    dS, dtaus, dtau2, dR8 = zeros(P * n, n), zeros(n, P), zeros(n, 1), zeros(n, n)
    torch.cuda.synchronize()
    for sh in range(P):
        sub = dA.data_ptr() + 8 * sh * ms
        ps.geqrf(sub, ms, n, m, dtaus.data_ptr() + 8 * n * sh)
        ps.extract_r(sub, ms, n, m, dS.data_ptr() + 8 * n * sh, n, P * n)       # R_s into rows [s n, (s+1) n) of the stack
    ps.sync()
    p2.geqrf(dS, P * n, n, P * n, dtau2)
    p2.extract_r(dS, P * n, n, P * n, dR8, n, n)
    p2.sync()
    R8 = host(dR8)
    assert rel(oracle.sign_normalise(R8), oracle.sign_normalise(R1)) < 1e-13
    ps.close(); p2.close()


@pytest.mark.parametrize("m,P", [(65536, 4), (262144, 2), (262144, 4)])
def test_c4_virtual_shards_match_single_factorisation(qr, oracle, m, P):
    """C4 on one device: P virtual row shards (the steps of the P-GPU run with a memcpy in place of the all-gather) give the same
    sign-normalised R as the unsharded factorisation -- at C4's full size 262144 x 256 with the shard heights of the 2- and
    4-GPU runs (131072, 65536), and at one shard's height."""
    n = 256
    A = qr.uniform_matrix_host(m, n, seed=12)
    Q1, R1 = qr.qr_thin(A, nb=128, nshards=1)
    Q4, R4 = qr.qr_thin(A, nb=128, nshards=P)
    assert rel(oracle.sign_normalise(R4), oracle.sign_normalise(R1)) < 1e-13
    assert rel(Q4 @ R4, A) < 1e-13 and np.abs(Q4.T @ Q4 - np.eye(n)).max() < 1e-12


def test_tall_skinny_65536x256_properties(qr):
    """One C4 shard (262144 x 256 over 4 GPUs -> 65536 x 256 per GPU)."""
    m, n = 65536, 256
    p = qr.Plan(m, n, 128, 32)
    dA = zeros(m, n)
    p.fill_uniform(dA, m, m, n, seed=12)
    p.sync()
    resid, orth, _ = _device_metrics(qr, p, dA, m, n, 12)
    assert resid < 1e-12 and orth < 1e-11
    p.close()


def test_geqrf_is_deterministic(qr):
    m, n = 3000, 512
    p = qr.Plan(m, n)
    outs = []
    for _ in range(2):
        dA, dtau = zeros(m, n), zeros(n, 1)
        p.fill_uniform(dA, m, m, n, seed=3)
        p.geqrf(dA, m, n, m, dtau)
        p.sync()
        outs.append((host(dA), host(dtau)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    p.close()


def test_calls_queued_without_a_sync_equal_synced_calls(qr):
    """geqrf, extract_r, applyq(identity) and a geqrf of a second matrix queued on one plan with a single sync at the end, against the same
    calls with a sync after each: the workspaces (panel sets, G, X, W, slabs) of the second factorisation meet the first one's wide update
    and the Q formation only through stream order and the schedule's events.  3920 x 2048 is the smallest shape (of whole 16-row tiles) at
    which the default plan takes look-ahead on a CU partition (n >= 2048, m n >= 8e6).  One deterministic schedule: bitwise equality."""
    m, n = 3920, 2048
    p = qr.Plan(m, n)
    assert p.info()[2] and 0 < p.update_cus() < 256          # look-ahead, and the wide update on its share of a partition

    def run(sync_each):
        dA, dB, dQ, dR, dR2 = zeros(m, n), zeros(m, n), zeros(m, n), zeros(n, n), zeros(n, n)
        dtau, dtau2 = zeros(n, 1), zeros(n, 1)
        p.fill_uniform(dA, m, m, n, seed=5)
        p.fill_uniform(dB, m, m, n, seed=6)
        p.sync()
        for call in (lambda: p.geqrf(dA, m, n, m, dtau), lambda: p.extract_r(dA, m, n, m, dR, n, n),
                     lambda: p.applyq(dA, m, n, m, dtau, dQ, n, m, True), lambda: p.geqrf(dB, m, n, m, dtau2),
                     lambda: p.extract_r(dB, m, n, m, dR2, n, n)):
            call()
            if sync_each:
                p.sync()
        p.sync()
        return host(dR), host(dQ), host(dR2)

    ref = run(True)
    got = run(False)
    assert np.isfinite(ref[0]).all() and np.abs(np.diag(ref[0])).min() > 0 and not np.array_equal(ref[0], ref[2])
    for name, a, b in zip(("R of the first matrix", "Q of the first matrix", "R of the second matrix"), got, ref):
        assert np.array_equal(a, b), f"{name}: {np.count_nonzero(a != b)} entries differ, max |diff| {np.abs(a - b).max():.3e}"
    p.close()


def test_profile_hooks(qr):
    m, n = 2048, 1024
    p = qr.Plan(m, n)
    dA, dtau = zeros(m, n), zeros(n, 1)
    p.fill_uniform(dA, m, m, n)
    p.set_profile(True)
    p.geqrf(dA, m, n, m, dtau)
    prof = p.get_profile()
    nb = qr.default_block_size(m, n)[0]
    assert 1 <= prof["update_nn"]["launches"] <= n // nb - 1 and prof["panel"]["launches"] == n // nb
    assert prof["update_nn"]["ms"] > 0 and prof["update_nn"]["flops"] > 0
    assert prof["update_nn"]["flops"] == prof["vta_tn"]["flops"]
    # class mask (what bench.py --full uses inside its timed region): only the wide update's class 0 carries events
    full_nn = prof["update_nn"]["launches"]
    p.fill_uniform(dA, m, m, n)
    p.set_profile(2 * (1 << 0))
    p.geqrf(dA, m, n, m, dtau)
    prof = p.get_profile()
    assert prof["update_nn"]["launches"] == full_nn and prof["update_nn"]["ms"] > 0
    assert prof["panel"]["launches"] == 0 and prof["vta_tn"]["launches"] == 0 and prof["vt_misc"]["launches"] == 0
    p.set_profile(2 * (1 << 2))
    p.fill_uniform(dA, m, m, n)
    p.geqrf(dA, m, n, m, dtau)
    prof = p.get_profile()
    assert prof["panel"]["launches"] == n // nb and prof["update_nn"]["launches"] == 0
    p.close()


@pytest.mark.parametrize("m,n", [(6, 4), (512, 128)])
def test_c_caller_links_the_drop_in_symbols(qr, tmp_path, m, n):
    """A plain C program written like the reference's main() (qr.c:461-523), compiled with gcc against
    include/mi355x_qr.h and linked to the shared library -- the drop-in boundary exercised from C."""
    import os, re, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "selfcheck")
    libdir = os.path.join(root, "cuda-qr_amd")
    subprocess.run(["gcc", "-std=c99", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "selfcheck.c"),
                    "-o", exe, "-L", libdir, "-lmi355xqr", "-lm", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([exe, str(m), str(n)], check=True, capture_output=True, text=True).stdout
    resid = float(re.search(r"L2 norm of residual QR-A: (\S+)", out).group(1))
    rel_resid = float(re.search(r"relative residual: (\S+)", out).group(1))
    assert rel_resid < 1e-12 and resid < 1e-12 * (m * n) ** 0.5 * 4
    if (m, n) == (6, 4):
        assert "Matrix 6 x 4, row by row:" in out          # printMat, qr.c:21-33


def test_qr_device_cli_like_reference_harness(qr):
    """`qr_device m n` (reference qr.cu:709-806): 3 timed host-pointer mmqr calls, average printed."""
    import os, re, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "cuda-qr_amd", "build", "qr_device")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(root, "cuda-qr_amd"), "build/qr_device"], check=True)
    out = subprocess.run([exe, "1024", "64"], check=True, capture_output=True, text=True, timeout=120).stdout
    assert "Exact problem size: 1024x64" in out
    m = re.search(r"MMQR ran QR on 1024x64 matrix in (\S+) s \(avg over 3\)", out)
    assert m and 0.0 < float(m.group(1)) < 5.0
    usage = subprocess.run([exe], capture_output=True, text=True)
    assert usage.returncode == 1 and "Usage: ./qr_device m n" in usage.stdout
    # --compare: the vendor line the reference prints under ENABLE_MAGMA (qr.cu:790-806), here rocSOLVER's dgeqrf
    try:
        out = subprocess.run([exe, "2048", "256", "--compare"], check=True, capture_output=True, text=True, timeout=45).stdout
    except subprocess.TimeoutExpired:
        pytest.skip("the vendor comparator (rocSOLVER through dlopen) did not finish within 45 s on this box")
    v = re.search(r"rocSOLVER ran QR on 2048x256 matrix in (\S+) s \(avg over 3\)", out)
    assert (v and 0.0 < float(v.group(1)) < 5.0) or "rocSOLVER not" in out


@pytest.mark.parametrize("m,n", [(1024, 1024), (2048, 2048), (1536, 1100), (3072, 3072)])
def test_dropin_roundtrip_where_the_default_block_is_not_the_global_one(qr, oracle, m, n):
    """mmqr -> explicitQR through the host-pointer ABI on shapes that get nb = 64 (small square-ish problems) or 256 (where the look-ahead
    schedule pays) by default while the global default stays 128: tau must carry all n scalars (it is sized from the block size the SHAPE gets) or explicitQR
    reads past it and returns a wrong Q."""
    rng = np.random.default_rng(m + n)
    A = rng.random((m, n))
    F, tau = qr.mmqr(A)
    assert tau.shape[0] == qr.tau_len(m, n) >= n
    assert np.all(tau[:n - 1] != 0.0)
    Q, R = qr.explicit_qr(F, tau)
    assert np.linalg.norm(A - Q @ R) / np.linalg.norm(A) < 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(m)) < 1e-12
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(F), ref) < 1e-13
    with pytest.raises(qr.QRError):
        qr.explicit_qr(F, tau[: n // 2])                 # a truncated tau is refused, not over-read


def test_dropin_roundtrip_f32_at_1024(qr):
    A = np.random.default_rng(9).random((1024, 1024)).astype(np.float32)
    F, tau = qr.mmqr_f32(A)
    assert tau.shape[0] == qr.tau_len(1024, 1024)
    Q, R = qr.explicit_qr_f32(F, tau)
    A64 = A.astype(np.float64)
    assert np.linalg.norm(Q.astype(np.float64) @ R.astype(np.float64) - A64) / np.linalg.norm(A64) < 1e-6


@pytest.mark.parametrize("plan_mn,sub_mn", [((16384, 2048), (8192, 2048)), ((16384, 2048), (4096, 2048)), ((12288, 1536), (3072, 1536))])
def test_subsize_geqrf_on_a_tall_plan(qr, oracle, plan_mn, sub_mn):
    """A plan made for m >= 8 n has the tall-skinny shortcut of the wide update (T applied to the small product, V*T never
    formed); a SMALLER problem on the same plan mixes slices that take the shortcut with slices that need V*T -- which must then
    be formed on demand (vt_formed) instead of being read stale from an older panel."""
    pm, pn = plan_mn
    m, n = sub_mn
    for la in ("0", "1"):
        import os
        os.environ["MI355XQR_LOOKAHEAD"] = la
        try:
            p = qr.Plan(pm, pn, 256, 32)
        finally:
            del os.environ["MI355XQR_LOOKAHEAD"]
        dA = zeros(m, n)
        p.fill_uniform(dA, m, m, n, seed=21)
        p.sync()
        A = host(dA)
        dtau, dR = zeros(n, 1), zeros(n, n)
        p.geqrf(dA, m, n, m, dtau)
        p.extract_r(dA, m, n, m, dR, n, n)
        p.sync()
        ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
        assert rel(oracle.sign_normalise(host(dR)), ref) < 1e-13, f"lookahead={la}"
        p.close()


@pytest.mark.parametrize("m_local,n,P", [(4096, 128, 1), (2048, 96, 3), (8192, 256, 4), (1000, 64, 2)])
def test_tsqr_plan_c_abi_virtual_ranks(qr, oracle, m_local, n, P):
    """The C-ABI device-resident TSQR step (qr_tsqr_plan_*) with P virtual ranks on ONE device: every rank's plan runs
    qr_tsqr_local_dev, the R factors are exchanged by the test through qr_tsqr_exchange_buffers (the hook for transports other
    than RCCL), qr_tsqr_stacked_dev gives the final R -- identical bits on every rank, equal to LAPACK's after sign
    normalisation -- and qr_tsqr_formq_dev the rank's rows of the thin Q.  P = 1 goes through qr_tsqr_factor_dev itself."""
    import ctypes as C
    m = m_local * P
    A = qr.uniform_matrix_host(m, n, seed=31)
    plans = [qr.TsqrPlan(m_local, n, P, r, 128, comm="external" if P > 1 else None) for r in range(P)]
    shards, Rs = [], []
    for r, tp in enumerate(plans):
        dA = zeros(m_local, n)
        tp.local.fill_uniform(dA, m_local, m_local, n, row_off=r * m_local, total_rows=m, seed=31)
        tp.sync()
        shards.append(dA)
        Rs.append(zeros(n, n))
    if P == 1:
        plans[0].factor(shards[0], m_local, Rs[0])
        assert plans[0].comm_ranks() == 1
    else:
        for tp, dA in zip(plans, shards):
            tp.local_factor(dA, m_local)
            tp.sync()
        nn8 = 8 * n * n
        for tp in plans:                                   # the "all-gather": rank q's send buffer -> slot q of every recv buffer
            _, recv = tp.exchange_buffers()
            for q, tq in enumerate(plans):
                send, _ = tq.exchange_buffers()
                tmp = np.empty(n * n)
                qr.check(qr.lib.qr_copy_to_host(tmp.ctypes.data, send, nn8))
                qr.check(qr.lib.qr_copy_to_device(recv + q * nn8, tmp.ctypes.data, nn8))
        for tp, dR in zip(plans, Rs):
            tp.stacked_factor(dR)
    for tp in plans:
        tp.sync()
    R0 = host(Rs[0])
    for dR in Rs[1:]:
        assert np.array_equal(R0, host(dR)), "every rank must hold the identical final R"
    assert np.array_equal(np.tril(R0, -1), np.zeros((n, n)))
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(R0), ref) < 1e-13
    Q = np.vstack([host(_formq(qr, tp, dA, m_local, n)) for tp, dA in zip(plans, shards)])
    assert np.linalg.norm(A - Q @ R0) / np.linalg.norm(A) < 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-12
    for tp in plans:
        tp.close()


def _formq(qr, tp, dA, m_local, n):
    dQ = zeros(m_local, n)
    tp.formq(dA, m_local, dQ, m_local)
    tp.sync()
    return dQ


def test_tsqr_plan_back_to_back_steps_are_stream_ordered(qr, oracle):
    """Independent factorisations issued back to back on one TSQR plan without any host synchronisation in between (the stacked
    QR of step i runs under the local QR of step i+1): every step's R must be the R of ITS matrix."""
    m_local, n, P = 16384, 128, 4
    tp = qr.TsqrPlan(m_local, n, P, 0, 128, comm="external")
    send, recv = tp.exchange_buffers()
    mats, Rs = [], []
    for i in range(4):
        dA = zeros(m_local, n)
        tp.local.fill_uniform(dA, m_local, m_local, n, seed=40 + i)
        mats.append(dA)
        Rs.append(zeros(n, n))
    tp.sync()
    hosts = [host(x) for x in mats]
    stream = qr.lib.qr_tsqr_stream(tp.h)
    for dA, dR in zip(mats, Rs):
        tp.local_factor(dA, m_local)
        # device-side "all-gather" of P copies of this rank's own factor, stream-ordered on the plan's stream
        for q in range(P):
            qr.check(qr.lib.qrd_copy_block(stream, send, n, recv + 8 * n * n * q, n, n, n))
        tp.stacked_factor(dR)
    tp.sync()
    for Ah, dR in zip(hosts, Rs):
        ref = oracle.sign_normalise(np.linalg.qr(np.vstack([np.linalg.qr(Ah, mode="r")] * P), mode="r"))
        assert rel(oracle.sign_normalise(host(dR)), ref) < 1e-13
    tp.close()


@pytest.mark.parametrize("m_local,n,P,nb", [(8192, 256, 4, 128), (4096, 512, 8, 128), (16384, 256, 2, 64), (65536, 256, 4, 128), (8192, 384, 3, 128)])
def test_tsqr_panel_pipelined_virtual_ranks(qr, oracle, m_local, n, P, nb):
    """The panel-pipelined TSQR step (block column k of every rank's R gathered as soon as local panel k is factored, the stacked
    matrix factored left-looking on a second stream while the local factorisation continues) with P virtual ranks on one device
    (qr_tsqr_factor_virtual_dev): every rank ends with the same R bit for bit, equal to LAPACK's R of the whole matrix after sign
    normalisation, and qr_tsqr_formq_dev on that left-looking factorisation gives the rank's rows of an orthonormal Q with QR = A."""
    m = m_local * P
    A = qr.uniform_matrix_host(m, n, seed=51)
    plans = [qr.TsqrPlan(m_local, n, P, r, nb, comm="external") for r in range(P)]
    assert all(tp.is_pipelined() for tp in plans)
    shards, Rs = [], []
    for r, tp in enumerate(plans):
        dA = zeros(m_local, n)
        tp.local.fill_uniform(dA, m_local, m_local, n, row_off=r * m_local, total_rows=m, seed=51)
        tp.sync()
        shards.append(dA)
        Rs.append(zeros(n, n))
    qr.tsqr_factor_virtual(plans, shards, m_local, Rs)
    R0 = host(Rs[0])
    for dR in Rs[1:]:
        assert np.array_equal(R0, host(dR)), "every rank must hold the identical final R"
    assert np.array_equal(np.tril(R0, -1), np.zeros((n, n)))
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(R0), ref) < 1e-13
    Q = np.vstack([host(_formq(qr, tp, dA, m_local, n)) for tp, dA in zip(plans, shards)])
    assert np.linalg.norm(A - Q @ R0) / np.linalg.norm(A) < 1e-13
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) < 1e-12
    for tp in plans:
        tp.close()


@pytest.mark.parametrize("heights,n,nb", [((9000, 8000, 8192, 7000), 512, 0), ((1500, 40000, 1100), 1024, 0), ((5000, 3000), 2048, 0)])
def test_tsqr_unequal_shards_agree_on_the_exchange(qr, oracle, heights, n, nb):
    """Shards of unequal height (m % ngpu != 0) used to straddle the look-ahead / block-size thresholds of the LOCAL plan, so that ranks
    disagreed on the number and size of the collectives (round-3 advisor finding).  A TSQR plan's local factorisation now takes a
    rank-invariant block size and the single-stream schedule: every rank reports the same pipelining decision and block size, and the
    virtual-rank run of the pipelined schedule over the unequal shards gives LAPACK's R on every rank."""
    P = len(heights)
    plans = [qr.TsqrPlan(h, n, P, r, nb, comm="external") for r, h in enumerate(heights)]
    assert len({tp.is_pipelined() for tp in plans}) == 1
    assert len({tp.local.nb for tp in plans}) == 1 and len({tp.stacked.nb for tp in plans}) == 1
    if not plans[0].is_pipelined():
        for tp in plans:
            tp.close()
        return
    rng = np.random.default_rng(sum(heights))
    hosts = [rng.random((h, n)) for h in heights]
    lda = max(heights)
    shards, Rs = [], []
    for Ah in hosts:
        buf = np.zeros((lda, n))
        buf[:Ah.shape[0]] = Ah
        shards.append(dev(buf))
        Rs.append(zeros(n, n))
    qr.tsqr_factor_virtual(plans, shards, lda, Rs)
    R0 = host(Rs[0])
    for dR in Rs[1:]:
        assert np.array_equal(R0, host(dR))
    ref = oracle.sign_normalise(np.linalg.qr(np.vstack(hosts), mode="r"))
    assert rel(oracle.sign_normalise(R0), ref) < 1e-13
    for tp in plans:
        tp.close()


def test_tsqr_selfgather_back_to_back_and_unpipelined_agree(qr, oracle, tmp_path):
    """One rank's complete step with its own factor in every rank slot (qr_tsqr_factor_selfgather_dev), issued back to back on four
    matrices without host synchronisation: every R is sqrt(P) times the R of ITS matrix; and the panel-pipelined schedule and the
    one-collective schedule (MI355XQR_TSQR_PIPE=0, child process) agree to rounding."""
    import subprocess, sys, os
    m_local, n, P = 32768, 256, 4
    tp = qr.TsqrPlan(m_local, n, P, 1, 128, comm="external")
    assert tp.is_pipelined()
    mats, Rs = [], []
    for i in range(4):
        dA = zeros(m_local, n)
        tp.local.fill_uniform(dA, m_local, m_local, n, seed=60 + i)
        mats.append(dA); Rs.append(zeros(n, n))
    tp.sync()
    hosts = [host(x) for x in mats]
    for dA, dR in zip(mats, Rs):
        tp.factor_selfgather(dA, m_local, dR)
    tp.sync()
    outs = []
    for Ah, dR in zip(hosts, Rs):
        ref = oracle.sign_normalise(np.linalg.qr(Ah, mode="r")) * np.sqrt(P)
        got = oracle.sign_normalise(host(dR))
        assert rel(got, ref) < 1e-13
        outs.append(got)
    tp.close()
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); import cuda_qr_amd as q\n"
            "tp = q.TsqrPlan(32768, 256, 4, 1, 128, comm='external'); assert not tp.is_pipelined()\n"
            "A = torch.zeros((256, 32768), dtype=torch.float64, device='cuda'); R = torch.zeros((256, 256), dtype=torch.float64, device='cuda'); torch.cuda.synchronize()\n"
            "tp.local.fill_uniform(A, 32768, 32768, 256, seed=60); tp.sync(); tp.factor_selfgather(A, 32768, R); tp.sync()\n"
            "np.save(sys.argv[1], R.cpu().numpy().T)\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "tsqr_unpiped.npy")
    subprocess.run([sys.executable, "-c", code, path], check=True, env=dict(os.environ, MI355XQR_TSQR_PIPE="0"))
    assert rel(oracle.sign_normalise(np.load(path)), outs[0]) < 1e-13


def test_tsqr_set_schedule_switches_between_the_two_exchange_forms_in_one_plan(qr, oracle):
    """qr_tsqr_set_schedule: one plan runs the panel-pipelined and the one-collective exchange (what bench.py --gpus N uses to print both
    schedules per rank).  Both give the same R; the gather statistics belong to the pipelined form only; mode 2 re-arms the library's rule;
    the diagnostic self-gather never takes part in the decision (three calls after mode 2 leave the plan pipelined)."""
    m_local, n, P = 32768, 256, 4
    tp = qr.TsqrPlan(m_local, n, P, 1, 128, comm="external")
    dA, dR = zeros(m_local, n), zeros(n, n)
    tp.local.fill_uniform(dA, m_local, m_local, n, seed=91)
    tp.sync()
    A0 = host(dA)
    ref = oracle.sign_normalise(np.linalg.qr(A0, mode="r")) * np.sqrt(P)
    got = {}
    for mode in (1, 0, 1, 2):
        tp.set_schedule(mode)
        assert tp.is_pipelined() == (mode != 0)
        dA.copy_(torch.from_numpy(np.ascontiguousarray(A0.T)).cuda())
        torch.cuda.synchronize()
        for _ in range(3 if mode == 2 else 1):
            tp.factor_selfgather(dA, m_local, dR)
            tp.sync()
            if mode == 2:
                dA.copy_(torch.from_numpy(np.ascontiguousarray(A0.T)).cuda()); torch.cuda.synchronize()
        got[mode] = oracle.sign_normalise(host(dR))
        assert rel(got[mode], ref) < 1e-13
        gs = tp.gather_stats()
        if mode == 0:
            assert not gs["pipelined"]
        else:
            assert gs["pipelined"] and gs["gather_ms"] > 0 and not gs["fell_back"]
    assert tp.is_pipelined()
    assert rel(got[0], got[1]) < 1e-13
    with pytest.raises(Exception):
        tp.set_schedule(3)
    tp.close()
    small = qr.TsqrPlan(4096, 64, 2, 0, 64, comm="external")       # one block column: the pipelined form does not exist for this shape
    assert not small.is_pipelined()
    with pytest.raises(Exception):
        small.set_schedule(1)
    small.set_schedule(0)
    small.close()


def test_tsqr_reserve_cus_masks_the_local_stream_and_changes_nothing_else(qr, oracle, tmp_path):
    """MI355XQR_TSQR_RESERVE_CUS=16 (child process: the knob is read at plan creation; rounded up to 32 = one CU per shader engine): the
    local factorisation of a multi-rank plan runs on a stream masked to 224 compute units -- the full-width panel sizes its launches to
    that -- and the result is LAPACK's."""
    import subprocess, sys, os
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); import cuda_qr_amd as q\n"
            "tp = q.TsqrPlan(65536, 256, 4, 1, 128, comm='external')\n"
            "A = torch.zeros((256, 65536), dtype=torch.float64, device='cuda'); R = torch.zeros((256, 256), dtype=torch.float64, device='cuda'); torch.cuda.synchronize()\n"
            "tp.local.fill_uniform(A, 65536, 65536, 256, seed=7); tp.sync(); A0 = A.cpu().numpy().T.copy()\n"
            "tp.factor_selfgather(A, 65536, R); tp.sync()\n"
            "np.save(sys.argv[1], R.cpu().numpy().T); np.save(sys.argv[2], A0)\n") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fR, fA = str(tmp_path / "tsqr_reserve_R.npy"), str(tmp_path / "tsqr_reserve_A.npy")
    subprocess.run([sys.executable, "-c", code, fR, fA], check=True,
                   env=dict(os.environ, MI355XQR_TSQR_RESERVE_CUS="16"), timeout=300)
    R, A0 = np.load(fR), np.load(fA)
    ref = oracle.sign_normalise(np.linalg.qr(A0, mode="r")) * 2.0          # sqrt(P) with the rank's own factor in every slot
    assert rel(oracle.sign_normalise(np.triu(R)), ref) < 1e-13


def test_tsqr_exchange_buffers_as_torch_views(qr, oracle):
    """The fallback transport of bench.py (torch.distributed gathers the R factors when the library cannot create its own RCCL
    communicator) works directly on the plan's device buffers through zero-copy torch views: the send view must show this rank's R
    after qr_tsqr_local_dev, and factors written through the recv view must be what qr_tsqr_stacked_dev factors."""
    from cuda_qr_amd import tsqr as T
    m_local, n, P = 4096, 96, 2
    tp = qr.TsqrPlan(m_local, n, P, 0, 32, comm="external")
    send, recv = tp.exchange_buffers()
    sv, rv = T._device_view(send, n * n, "cuda"), T._device_view(recv, P * n * n, "cuda")
    assert sv.data_ptr() == send and rv.data_ptr() == recv
    A = qr.uniform_matrix_host(2 * m_local, n, seed=77)
    dA = dev(A[:m_local])
    tp.local_factor(dA, m_local)
    tp.sync()
    R0 = np.triu(sv.cpu().numpy().reshape(n, n).T)
    ref0 = oracle.sign_normalise(np.linalg.qr(A[:m_local], mode="r"))
    assert rel(oracle.sign_normalise(R0), ref0) < 1e-13
    R1 = np.linalg.qr(A[m_local:], mode="r")
    rv[: n * n].copy_(sv)
    rv[n * n:].copy_(torch.from_numpy(np.ascontiguousarray(np.triu(R1).T).ravel()).cuda())
    torch.cuda.synchronize()
    dR = zeros(n, n)
    tp.stacked_factor(dR)
    tp.sync()
    ref = oracle.sign_normalise(np.linalg.qr(A, mode="r"))
    assert rel(oracle.sign_normalise(host(dR)), ref) < 1e-13
    tp.close()


_GRAPH_CHILD = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r)
import cuda_qr_amd as qr
from oracle import oracle as O          # the checker: sign normalisation only
assert qr.LAB
for (m, n, nb, la) in [(3000, 700, 128, "0"), (40000, 256, 128, "0"), (2500, 2304, 128, "1")]:
    os.environ["MI355XQR_LOOKAHEAD"] = la        # read at plan creation
    p = qr.Plan(m, n, nb, 32)
    dA = torch.zeros((n, m), dtype=torch.float64, device="cuda"); dtau = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    dR = torch.zeros((n, n), dtype=torch.float64, device="cuda"); torch.cuda.synchronize()
    for seed in (3, 4, 5):
        p.fill_uniform(dA, m, m, n, seed=seed)
        p.sync()
        p.geqrf(dA, m, n, m, dtau)
        p.extract_r(dA, m, n, m, dR, n, n)
        p.sync()
        ref = O.sign_normalise(np.linalg.qr(qr.uniform_matrix_host(m, n, seed=seed), mode="r"))
        got = O.sign_normalise(np.asfortranarray(dR.cpu().numpy().T))
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-13, (m, n, la, seed)
    p.close()
"""


def test_graph_replay_single_stream_schedule(qr):
    """MI355XQR_GRAPH=1 (a measurement knob: lab library, child process): the single-stream schedule is captured into a hipGraph on the
    first call with an argument set and replayed afterwards -- three different matrices through the same buffer must each give their
    own R; with look-ahead the knob is ignored (capturing the CU-masked two-stream schedule crashes inside the runtime)."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", _GRAPH_CHILD % root], check=True, timeout=600,
                   env=dict(os.environ, CUDA_QR_AMD_LIB="lab", MI355XQR_GRAPH="1"))
