"""The extended-precision reference of the GPU accuracy tests (tests/hp_ref.py) checked on the CPU: its float64 instance against
numpy / LAPACK to the textbook bound, bitwise equivariance of that instance under powers of two (the property
tests/test_gpu_scale_equivariance.py asks of every kernel), and the longdouble instance's residuals at longdouble round-off.

Bounds: for an m x n Householder QR the backward error is c m n eps with a small c (Higham, Accuracy and Stability, Thm 19.4); the
checks use m eps for ||A - QR|| / ||A|| and ||Q^T Q - I||_F / sqrt(n) at float64, and 100 eps_longdouble for the longdouble
instance's residuals (measured: at most 3.3 eps_longdouble for ||A - QR|| / ||A||, 36.7 for ||Q^T Q - I||_F at 300 x 128, below 1 for
the solves).  R against LAPACK: 50 kappa eps as tests/test_gpu_update.py.
"""
import functools

import numpy as np
import pytest

import hp_ref as H

EPS = H.EPS
SHAPES = [(300, 128), (65, 63), (7, 1)]
SCALES = [2.0 ** 40, 2.0 ** -40, 2.0 ** 301, 2.0 ** -299]


@functools.lru_cache(maxsize=None)
def _inputs(m, n):
    rng = np.random.default_rng(100 * m + n)
    A, B = rng.random((m, n)) - 0.5, rng.random((m, 3)) - 0.5
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


@pytest.mark.parametrize("m,n", SHAPES)
def test_float64_instance_agrees_with_numpy(m, n):
    A, B = _inputs(m, n)
    F, tau = H.qr(A, np.float64)
    assert F.dtype == np.float64 and tau.dtype == np.float64
    R, Q = H.triu(F), H.form_q(F, tau, np.float64)
    Rl = np.linalg.qr(A, mode="r")
    sg = np.sign(np.diag(Rl)) * np.sign(np.diag(R))
    kappa = np.linalg.cond(A)
    assert np.linalg.norm(R - sg[:, None] * Rl) <= 50 * kappa * EPS * np.linalg.norm(Rl)
    assert R[0, 0] * A[0, 0] < 0                                            # dlarfg: beta has the sign opposite to alpha
    assert np.linalg.norm(A - Q @ R) <= m * EPS * np.linalg.norm(A)
    assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= m * EPS * np.sqrt(n)
    # apply: Q^T A = [R; 0], and 'N' undoes 'T'
    QtA = H.apply_q(F, tau, A, "T", np.float64)
    assert np.linalg.norm(QtA[:n] - R) <= m * EPS * np.linalg.norm(A) and np.linalg.norm(QtA[n:]) <= m * EPS * np.linalg.norm(A)
    assert np.linalg.norm(H.apply_q(F, tau, QtA, "N", np.float64) - A) <= m * EPS * np.linalg.norm(A)
    # substitutions
    Y = B[:n]
    for X, M in ((H.solve_r(R, Y, np.float64), R), (H.solve_rt(R, Y, np.float64), R.T)):
        assert np.linalg.norm(M @ X - Y) <= n * EPS * (np.linalg.norm(R) * np.linalg.norm(X) + np.linalg.norm(Y))
    # least squares and minimum norm
    X, res = H.lstsq(A, B, np.float64)
    Xl = np.linalg.lstsq(A, B, rcond=None)[0]
    nA = np.linalg.norm(A)
    bound = 50 * EPS * (kappa + kappa ** 2 * np.linalg.norm(A @ Xl - B) / (nA * np.linalg.norm(Xl)))
    assert np.linalg.norm(X - Xl) <= bound * np.linalg.norm(Xl)
    assert np.allclose(res, np.linalg.norm(A @ Xl - B, axis=0), rtol=1e-12, atol=m * EPS * np.linalg.norm(B))
    W, C = A.T, B[:n]
    Z = H.minnorm(W, C, np.float64)
    Zl = np.linalg.lstsq(W, C, rcond=None)[0]
    assert np.linalg.norm(Z - Zl) <= 50 * kappa * EPS * np.linalg.norm(Zl)


@pytest.mark.parametrize("m,n", SHAPES)
def test_float64_update_removal_and_pivoting_agree_with_numpy(m, n):
    A, _ = _inputs(m, n)
    kappa = np.linalg.cond(A)
    h = max(n, m // 2)
    R0 = H.triu(H.qr(A[:h], np.float64)[0])
    Fa, _ = H.append_rows(R0, A[h:], np.float64)
    Rl = np.linalg.qr(A, mode="r")
    for R in (H.triu(Fa), H.remove_rows(np.vstack([A, A[:3]]), np.arange(m), np.float64)):
        sg = np.sign(np.diag(Rl)) * np.sign(np.diag(R))
        assert np.linalg.norm(R - sg[:, None] * Rl) <= 50 * kappa * EPS * np.linalg.norm(Rl)
    F, tau, jp = H.qrp(A, np.float64)
    Q, R = H.form_q(F, tau, np.float64), H.triu(F)
    assert sorted(jp) == list(range(n))
    assert np.linalg.norm(A[:, jp] - Q @ R) <= m * EPS * np.linalg.norm(A)
    d = np.abs(np.diag(R))
    assert np.all(d[1:] <= d[:-1] * (1 + 100 * np.sqrt(EPS)))
    # an exactly dependent column ends last with a negligible diagonal
    if n >= 3:
        A2 = A.copy()
        A2[:, 1] = 2 * A2[:, 0] - A2[:, 2]
        F2, _, jp2 = H.qrp(A2, np.float64)
        assert abs(F2[n - 1, n - 1]) <= m * EPS * abs(F2[0, 0])


@pytest.mark.parametrize("m,n", SHAPES)
@pytest.mark.parametrize("s", SCALES)
def test_float64_instance_is_bitwise_equivariant(m, n, s):
    A, B = _inputs(m, n)
    t = 2.0 ** -77
    f64 = np.float64
    F, tau = H.qr(A, f64)
    Fs, taus = H.qr(s * A, f64)
    R, Rs = H.triu(F), H.triu(Fs)
    assert np.array_equal(np.tril(Fs, -1), np.tril(F, -1)) and np.array_equal(Rs / s, R) and np.array_equal(taus, tau)
    assert np.array_equal(H.form_q(Fs, taus, f64), H.form_q(F, tau, f64))
    assert np.array_equal(H.apply_q(Fs, taus, t * B, "T", f64) / t, H.apply_q(F, tau, B, "T", f64))
    Y = B[:n]
    assert np.array_equal(H.solve_r(Rs, t * Y, f64) * (s / t), H.solve_r(R, Y, f64))
    assert np.array_equal(H.solve_rt(Rs, t * Y, f64) * (s / t), H.solve_rt(R, Y, f64))
    X, res = H.lstsq(A, B, f64)
    Xs, ress = H.lstsq(s * A, t * B, f64)
    assert np.array_equal(Xs * (s / t), X) and np.array_equal(ress / t, res)
    assert np.array_equal(H.minnorm(s * A.T, t * Y, f64) * (s / t), H.minnorm(A.T, Y, f64))
    h = max(n, m // 2)
    assert np.array_equal(H.triu(H.append_rows(Rs, s * A[h:], f64)[0]) / s, H.triu(H.append_rows(R, A[h:], f64)[0]))
    Fp, taup, jp = H.qrp(A, f64)
    Fps, taups, jps = H.qrp(s * A, f64)
    assert np.array_equal(jps, jp) and np.array_equal(taups, taup)
    assert np.array_equal(np.tril(Fps, -1), np.tril(Fp, -1)) and np.array_equal(H.triu(Fps) / s, H.triu(Fp))


@pytest.mark.parametrize("m,n", SHAPES)
def test_longdouble_instance_residuals(m, n):
    A, B = _inputs(m, n)
    F, tau = H.qr(A)
    Q, R = H.form_q(F, tau), H.triu(F)
    resid, orth = H.factor_errors(A, Q, R)
    X, _ = H.lstsq(A, B)
    ne = H.normal_equations_residual(A, X, B)
    Y = B[:n]
    b1 = H.trsm_backward_error(R, H.solve_r(R, Y), Y)
    b2 = H.trsm_backward_error(R, H.solve_rt(R, Y), Y, trans=True)
    print(f"hp_ref longdouble {m}x{n}: resid {resid / H.EPS_LD:.1f} orth {orth / H.EPS_LD:.1f} normal-eq {ne / H.EPS_LD:.1f} "
          f"trsm {b1 / H.EPS_LD:.1f} / {b2 / H.EPS_LD:.1f} (eps_ld)")
    assert resid < 100 * H.EPS_LD and orth < 100 * H.EPS_LD
    assert ne < 100 * H.EPS_LD and b1 < 100 * H.EPS_LD and b2 < 100 * H.EPS_LD
    # and the float64 instance of the same code sits at float64 round-off, far above it: the two are distinguishable
    F64, tau64 = H.qr(A, np.float64)
    r64, o64 = H.factor_errors(A, H.form_q(F64, tau64, np.float64), H.triu(F64))
    assert 100 * H.EPS_LD < max(r64, o64) <= m * EPS * np.sqrt(n)
