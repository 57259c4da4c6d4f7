"""-m gpu: singular values, SVD and minimum-norm least squares (mi355x_qr.h section 7) against numpy / LAPACK.

Singular vectors are never compared with numpy's (signs and degenerate subspaces differ): values, reconstruction and orthogonality are.
With s = the sweeps the call reports, n s eps is the first-order worst case for a column that passes through (n - 1) s rotations:
    ||G - U S V^T||_F / ||G||_F <= s n eps,   max |sigma_i - sigma_i(numpy)| / sigma_0 <= s n eps,
    ||V^T V - I||_F, ||U_k^T U_k - I||_F <= 4 s n eps      (U_k: the columns with sigma_i > n eps sigma_0)
and s <= 20 (a CPU emulation of the algorithm needed at most 11 on these inputs; an inner solve that breaks convergence shows as 30).
Column norms are measured with math.fsum, so that the 4 eps bound on them is not spent on the measurement.
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from gpu_util import dev, host, rel, zeros
from test_gpu_lstsq import _check
from test_gpu_pivot import _cond_matrix
from test_gpu_update import _strided, _unstrided

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENT = -3.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _uniform(r, n):
    A = np.random.default_rng(100 * r + n).random((r, n)) - 0.5
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def _np_svals(r, n):
    return np.linalg.svd(_uniform(r, n), compute_uv=False)


def _vec(n):
    t = torch.full((n + 2,), SENT, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    return t, t[1:]


def _vec_out(t, n):
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert h[0] == SENT and h[n + 1] == SENT, "written outside dS"
    return h[1:n + 1].copy()


def _mat_out(t, m, n, ld, off=1):
    h = t.cpu().numpy()
    assert np.all(h[:off] == SENT) and np.all(h[off:].reshape(n, ld)[:, m:] == SENT), "written outside the matrix"
    return _unstrided(t, m, n, ld, off)


def _gesvj(plan, G, jobv="V"):
    """qr_gesvj_dev on odd leading dimensions, bases one double off, sentinel fill: (U, S, V or None, sweeps)"""
    r, n = G.shape
    ldg, ldv = (r + 2) | 1, (n + 2) | 1
    tG, dG = _strided(G, ldg, 1, SENT)
    tS, dS = _vec(n)
    tV, dV = _strided(np.full((n, n), 3.0), ldv, 1, SENT) if jobv == "V" else (None, None)
    sw = plan.gesvj(jobv, dG, r, n, ldg, dS, dV, ldv if jobv == "V" else 0)
    plan.sync()
    return _mat_out(tG, r, n, ldg), _vec_out(tS, n), (_mat_out(tV, n, n, ldv) if jobv == "V" else None), sw


def _orth(X):
    return np.linalg.norm(X.T @ X - np.eye(X.shape[1]))


def _col_norms(X):
    return np.array([math.sqrt(math.fsum(c * c)) for c in X.T])


def _check_svd(tag, G, U, S, V, sw, Snp, extra_rec=0.0, extra_u=0.0):
    n = G.shape[1]
    unit = sw * n * EPS
    assert np.all(np.isfinite(U)) and np.all(np.isfinite(S)) and np.all(np.isfinite(V))
    assert np.all(S >= 0.0) and np.all(np.diff(S) <= 0.0), "dS is not descending / non-negative"
    rec = np.linalg.norm(G - (U * S) @ V.T) / np.linalg.norm(G)
    sig = np.max(np.abs(S - Snp)) / Snp[0]
    ov = _orth(V)
    k = int(np.sum(S > n * EPS * S[0]))
    ou = _orth(U[:, :k])
    print(f"{tag}: sweeps {sw}, in units of n eps: reconstruction {rec / (n * EPS):.2f}, sigma {sig / (n * EPS):.2f}, "
          f"V^T V - I {ov / (n * EPS):.2f}, U^T U - I {ou / (n * EPS):.2f} (k = {k})")
    assert sw <= 20
    assert rec <= unit + extra_rec
    assert sig <= unit
    assert ov <= 4 * unit
    assert ou <= 4 * unit + extra_u
    return k


SHAPES = [(20, 20), (33, 33), (64, 64), (96, 96), (200, 200), (300, 96), (330, 330)]


@pytest.mark.parametrize("r,n", SHAPES)
def test_gesvj_values_vectors_extents_and_determinism(qr, r, n):
    G = _uniform(r, n)
    plan = qr.Plan(r, n, 0, 0)
    U, S, V, sw = _gesvj(plan, G)
    k = _check_svd(f"gesvj {r}x{n}", G, U, S, V, sw, _np_svals(r, n))
    assert k == n
    nu = np.max(np.abs(_col_norms(U) - 1.0))
    print(f"  column norms of U: {nu / EPS:.2f} eps from 1 (bound 4)")
    assert nu <= 4 * EPS
    U2, S2, V2, sw2 = _gesvj(plan, G)
    assert np.array_equal(U, U2) and np.array_equal(S, S2) and np.array_equal(V, V2) and sw == sw2
    plan.close()


def test_gesvj_values_only_is_bitwise_the_same(qr):
    G = _uniform(200, 200)
    plan = qr.Plan(200, 200, 0, 0)
    _, S, _, sw = _gesvj(plan, G)
    _, S0, V0, sw0 = _gesvj(plan, G, jobv="N")          # dV = NULL
    assert V0 is None and sw0 == sw and np.array_equal(S, S0)
    plan.close()


def test_gesvj_diagonal_input_takes_one_sweep_and_is_exact(qr):
    n = 96
    d = np.random.default_rng(5).random(n) + 0.5        # distinct, positive, in no order
    plan = qr.Plan(n, n, 0, 0)
    U, S, V, sw = _gesvj(plan, np.diag(d))
    order = np.argsort(-d, kind="stable")
    P = np.zeros((n, n))
    P[order, np.arange(n)] = 1.0
    assert sw == 1
    assert np.array_equal(S, d[order]), "the sorted diagonal, exactly"
    assert np.array_equal(V, P) and np.array_equal(U, P), "permutation matrices, exactly"
    plan.close()


def test_gesvj_zero_columns_stay_zero(qr):
    n = 64
    G = np.array(_uniform(n, n))
    G[:, 5] = 0.0
    G[:, 40] = 0.0
    plan = qr.Plan(n, n, 0, 0)
    U, S, V, sw = _gesvj(plan, G)
    assert np.all(S[-2:] == 0.0) and S[-3] > 0.0
    assert np.all(U[:, -2:] == 0.0), "a zero singular value goes with an exact zero column"
    k = _check_svd("gesvj 64x64, two zero columns", G, U, S, V, sw, np.linalg.svd(G, compute_uv=False))
    assert k == n - 2
    assert np.max(np.abs(_col_norms(U[:, :k]) - 1.0)) <= 4 * EPS
    plan.close()


def test_gesvj_zero_matrix(qr):
    n = 33
    plan = qr.Plan(n, n, 0, 0)
    U, S, V, sw = _gesvj(plan, np.zeros((n, n)))
    assert sw == 1 and np.all(S == 0.0) and np.all(U == 0.0) and np.array_equal(V, np.eye(n))
    plan.close()


def _gesvd(qr, A, jobs="UV"):
    """qr_gesvd_dev on odd leading dimensions and bases one double off: (U, S, V, sweeps, R of the factors left in dA)"""
    m, n = A.shape
    lda, ldu, ldv = (m + 2) | 1, (m + 4) | 1, (n + 2) | 1
    plan = qr.Plan(m, n, 0, 0)
    tA, dA = _strided(A, lda, 1, SENT)
    tS, dS = _vec(n)
    dtau = zeros(n, 1)
    U = V = None
    if jobs == "UV":
        tU, dU = _strided(np.full((m, n), 3.0), ldu, 1, SENT)
        tV, dV = _strided(np.full((n, n), 3.0), ldv, 1, SENT)
        sw = plan.gesvd("U", "V", dA, m, n, lda, dtau, dS, dU, ldu, dV, ldv)
    else:
        sw = plan.gesvd("N", "N", dA, m, n, lda, dtau, dS)
    dR = zeros(n, n)
    plan.extract_r(dA, m, n, lda, dR, n, n)
    plan.sync()
    if jobs == "UV":
        U, V = _mat_out(tU, m, n, ldu), _mat_out(tV, n, n, ldv)
    S, R = _vec_out(tS, n), host(dR)
    plan.close()
    return U, S, V, sw, R


@pytest.mark.parametrize("m,n", [(70, 33), (1000, 96), (3000, 200), (5001, 330)])
def test_gesvd_tall(qr, m, n):
    A = _uniform(m, n)
    U, S, V, sw, R = _gesvd(qr, A)
    # 1e-12: the bound test_gpu_qr.py puts on the factorisation's own residual; 4e-12 sqrt(m): its bound on Q
    _check_svd(f"gesvd {m}x{n}", A, U, S, V, sw, _np_svals(m, n), extra_rec=1e-12, extra_u=4e-12 * np.sqrt(m))
    _, S0, _, sw0, _ = _gesvd(qr, A, jobs="NN")
    assert sw0 == sw and np.array_equal(S, S0), "values only: the same rotations, no accumulation"
    g = np.linalg.norm(R.T @ R - A.T @ A) / np.linalg.norm(A.T @ A)
    print(f"  factors left in dA: ||R^T R - A^T A|| / ||A^T A|| = {g / (n * EPS):.2f} n eps (bound 10)")
    assert np.all(np.tril(R, -1) == 0.0) and g <= 10 * n * EPS


def test_prescribed_spectrum_and_condition_number(qr):
    m, n = 2000, 200
    A = _cond_matrix(m, n, 1e10, 7)
    want = np.logspace(0, -10, n)
    _, S, _, sw, _ = _gesvd(qr, A, jobs="NN")
    e = np.max(np.abs(S - want)) / want[0]
    print(f"cond 1e10 spectrum: sweeps {sw}, sigma error {e / (n * EPS):.2f} n eps (bound {sw})")
    assert sw <= 20 and e <= sw * n * EPS
    plan = qr.Plan(m, n, 0, 0)
    c = plan.cond(dev(A), m, n, m, zeros(n, 1))
    # sigma_min = 1e-10 carries an absolute error of up to s n eps sigma_0: that relative to it, twice over, once s exceeds 2
    bound = 1e-3 if sw <= 2 else 2 * sw * n * EPS * 1e10
    print(f"  qr_cond_dev / 1e10 - 1 = {c / 1e10 - 1:.3e} (bound {bound:.3e})")
    assert abs(c / 1e10 - 1.0) <= bound
    Z = np.array(_uniform(300, 40))
    Z[:, 17] = 0.0
    assert plan.cond(dev(Z), 300, 40, 300, zeros(40, 1)) == np.inf
    plan.close()


@functools.lru_cache(maxsize=None)
def _deficient():
    """1500 x 120 of rank 115: 115 columns of condition 1e3 and 5 fixed combinations of the first five"""
    A1 = _cond_matrix(1500, 115, 1e3, 21)
    Cm = np.array([[1.0, 0.5, 0.0, -1.0, 2.0], [0.0, 1.0, 1.0, 0.5, -0.5], [2.0, 0.0, -1.0, 1.0, 0.0], [-1.0, 1.5, 0.0, 1.0, 1.0],
                   [0.5, 0.0, 2.0, 0.0, -1.0]])
    A = np.hstack([A1, A1[:, :5] @ Cm])
    s = np.linalg.svd(A, compute_uv=False)
    A.setflags(write=False)
    return A, s[0] / s[114]


def test_gelss_minimum_norm_on_a_rank_deficient_matrix(qr):
    A, kappa = _deficient()
    m, n = A.shape
    assert kappa <= 2e4
    _, _, _, sw, _ = _gesvd(qr, A, jobs="NN")            # the sweeps of the same iteration (qr_gelss_dev does not report them)
    assert sw <= 20
    rng = np.random.default_rng(3)
    # (a) consistent, on the device API
    B = A @ rng.standard_normal((n, 3))
    Xn = np.linalg.lstsq(A, B, rcond=1e-10)[0]
    plan = qr.Plan(m, n, 0, 0)
    dA, dB, dS = dev(A), dev(B), zeros(n, 1)
    rank = plan.gelss(dA, m, n, m, zeros(n, 1), dB, 3, m, dS, rcond=1e-10)
    plan.sync()
    X = host(dB)[:n]
    e = rel(X, Xn)
    print(f"gelss consistent: rank {rank}, sweeps {sw}, |X - X_np| / |X_np| = {e:.2e} (bound {10 * kappa * sw * n * EPS:.2e}, kappa_r {kappa:.0f})")
    assert rank == 115 and e <= 10 * kappa * sw * n * EPS
    plan.close()
    X2, _, rank2, S2 = qr.lstsq_svd(A, B, rcond=1e-10)
    assert rank2 == 115 and rel(X2, Xn) <= 10 * kappa * sw * n * EPS
    assert np.array_equal(S2, qr.svdvals(A)), "the values of the accumulating and the values-only path are bitwise the same"
    # (b) noisy
    Bn = B + 0.1 * rng.standard_normal(B.shape)
    Xn = np.linalg.lstsq(A, Bn, rcond=1e-10)[0]
    X, resid, rank, _ = qr.lstsq_svd(A, Bn, rcond=1e-10)
    Xb, _, rb, _ = qr.lstsq_pivoted(A, Bn, rcond=1e-10)
    assert rank == 115 and rb == 115
    for j in range(3):
        r, rn = np.linalg.norm(A @ X[:, j] - Bn[:, j]), np.linalg.norm(A @ Xn[:, j] - Bn[:, j])
        x, xn, xb = np.linalg.norm(X[:, j]), np.linalg.norm(Xn[:, j]), np.linalg.norm(Xb[:, j])
        print(f"gelss noisy, column {j}: residual / numpy's - 1 = {r / rn - 1:.2e}, |x| / |x_np| - 1 = {x / xn - 1:.2e}, basic |x| = {xb / x:.3f} |x|")
        assert r <= (1 + 1e-10) * rn and x <= (1 + 1e-8) * xn
        assert abs(resid[j] - rn) <= 1e-10 * rn      # the discarded components carry s n eps |b| ~ 3e-12 |r| here; 30 times that
        assert xb > x, "the basic solution of section 4 is longer than the minimum-norm one"


def test_lstsq_svd_full_rank_and_zero_matrix(qr):
    A = _uniform(1000, 96)
    B = np.random.default_rng(8).random((1000, 2)) - 0.5
    X, resid, rank, S = qr.lstsq_svd(A, B)
    assert rank == 96
    _check(A, B, X, resid, S[0] / S[-1])
    X1, r1 = qr.lstsq(A, B)
    assert rel(X, X1) <= 1e-12
    X, resid, rank, S = qr.lstsq_svd(np.zeros((50, 20)), B[:50])
    assert rank == 0 and np.all(X == 0.0) and np.all(S == 0.0)
    assert np.allclose(resid, np.linalg.norm(B[:50], axis=0), rtol=1e-13)


def test_host_twins_and_tool(qr):
    m, n = 1000, 96
    A = np.array(_uniform(m, n))
    A0 = A.copy()
    U, S, V = qr.svd(A)
    assert np.array_equal(A, A0), "A is the caller's"
    _, _, _, sw, _ = _gesvd(qr, A, jobs="NN")
    _check_svd(f"qr.svd {m}x{n}", A, U, S, V, sw, _np_svals(m, n), extra_rec=1e-12, extra_u=4e-12 * np.sqrt(m))
    assert np.array_equal(qr.svdvals(A), S) and np.array_equal(qr.svd(A, compute_uv=False), S)
    assert qr.cond(A) == S[0] / S[-1]
    out = subprocess.run([os.path.join(ROOT, "cuda-qr_amd", "build", "qr_device"), "2000", "200", "--svd"], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    line = [l for l in out.stdout.splitlines() if "||A - U S V^T||" in l][0]
    assert float(line.split("=")[1].split()[0]) < 1e-12
    assert "sigma_max" in out.stdout and "sweeps" in out.stdout
