"""The extended-precision reference of the GPU accuracy tests (tests/hp_ref.py) checked on the CPU: its float64 instance against
numpy / LAPACK to the textbook bound, bitwise equivariance of that instance under powers of two (the property
tests/test_gpu_scale_equivariance.py asks of every kernel), and the longdouble instance's residuals at longdouble round-off.

Bounds: for an m x n Householder QR the backward error is c m n eps with a small c (Higham, Accuracy and Stability, Thm 19.4); the
checks use m eps for ||A - QR|| / ||A|| and ||Q^T Q - I||_F / sqrt(n) at float64, and 100 eps_longdouble for the longdouble
instance's residuals (measured: at most 3.3 eps_longdouble for ||A - QR|| / ||A||, 36.7 for ||Q^T Q - I||_F at 300 x 128, below 1 for
the solves).  R against LAPACK: 50 kappa eps as tests/test_gpu_update.py.

The launch-layer references: the unsigned tp_panel is append_rows to 1e-18 relative (measured: 1.0e-19), the signed one satisfies
R'^T R' = R^T R + B^T S B, I - U T U^T Phi is the product of the single reflectors and tp_apply its transposed action, all to 1000
eps_longdouble (times the cancellation of the Gram identity, times kappa(R') where R' is recovered); jacobi_pair's J is orthogonal to
1000 eps_longdouble (measured: 56) and its output's measure, recomputed in longdouble, is at most tol.
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


# ---- the launch-layer references: tp_panel / tp_apply (csrc/qr_update.hip) and jacobi_pair (csrc/qr_svd.hip) --------------------------
PANEL_SHAPES = [(32, 256), (32, 70), (7, 65), (1, 1), (31, 100)]


@functools.lru_cache(maxsize=None)
def _panel_inputs(w, p):
    """R = the triangle of numpy's QR of a random 2w x w matrix, B uniform in [-0.5, 0.5), as tests/test_gpu_update.py builds them"""
    rng = np.random.default_rng(1000 * w + p)
    R = np.triu(np.linalg.qr(rng.random((2 * w, w)) - 0.5, mode="r"))
    B = rng.random((p, w)) - 0.5
    return R, B


@functools.lru_cache(maxsize=None)
def _signed_inputs(w, p, p_add):
    """R of standard-normal rows of which the block's last p - p_add are removed again (d > 0 with margin), as tests/test_gpu_downdate.py"""
    rng = np.random.default_rng(7000 + 1000 * w + 10 * p_add + p)
    rows = rng.standard_normal((2 * w + p - p_add, w))
    R = np.triu(np.linalg.qr(rows, mode="r"))
    return R, np.vstack([rng.standard_normal((p_add, w)), rows[:p - p_add]])


def _relerr(X, Y):
    return float(H.norm(H.arr(X) - H.arr(Y)) / H.norm(Y))


@pytest.mark.parametrize("w,p", PANEL_SHAPES)
def test_unsigned_tp_panel_is_append_rows(w, p):
    R, B = _panel_inputs(w, p)
    Rn, V, T = H.tp_panel(R, B)
    F, tau = H.append_rows(R, B)
    e = max(_relerr(Rn, H.triu(F)), _relerr(V, F[w:]), _relerr(np.diag(T), tau))
    print(f"tp_panel {w}x{p} against append_rows: {e:.2e}")
    assert e <= 1e-18
    assert not np.any(np.tril(T, -1) != 0)
    # the float64 instance sits at float64 round-off of the longdouble one
    R64, V64, T64 = H.tp_panel(R, B, dtype=np.float64)
    assert R64.dtype == np.float64 and 1e-18 < _relerr(R64, Rn) <= 50 * np.linalg.cond(np.vstack([R, B])) * EPS
    assert _relerr(V64, V) <= (w + p) * EPS and _relerr(T64, T) <= (w + p) * EPS


@pytest.mark.parametrize("w,p,p_add", [(32, 256, 0), (32, 70, 37), (32, 70, 5), (7, 65, 64), (31, 100, 50), (1, 1, 0)])
def test_signed_tp_panel_gram_identity_and_compact_form(w, p, p_add):
    R, B = _signed_inputs(w, p, p_add)
    Rn, V, T = H.tp_panel(R, B, p_add)
    s = np.where(np.arange(p) < p_add, 1.0, -1.0)
    G = H.matmul(R.T, R) + H.matmul(B.T, s[:, None] * B)
    assert _relerr(H.matmul(Rn.T, Rn), G) <= 1000 * H.EPS_LD * float(H.norm(H.matmul(R.T, R)) / H.norm(G))
    # I - U T U^T Phi is the product of the single reflectors Theta_j = I - tau_j u_j u_j^T Phi, u_j = [e_j ; V(:, j)], Phi = diag(I, S)
    U = H.arr(np.vstack([np.eye(w), np.zeros((p, w))]))
    U[w:] = V
    phi = H.arr(np.concatenate([np.ones(w), s]))
    Q = H.arr(np.eye(w + p))
    for j in range(w):
        Q = Q - T[j, j] * H.matmul(H.matmul(Q, U[:, j][:, None]), (U[:, j] * phi)[None, :])
    C = H.arr(np.eye(w + p)) - H.matmul(H.matmul(U, T), (U * phi[:, None]).T)
    assert float(H.norm(Q - C)) <= 1000 * H.EPS_LD * float(H.norm(Q))
    # and tp_apply is that operator's transposed action: [C1 ; C2] <- (I - U T^T U^T Phi) [C1 ; C2]
    rng = np.random.default_rng(w + p)
    C1, C2 = rng.standard_normal((w, 3)), rng.standard_normal((p, 3))
    A1, A2 = H.tp_apply(V, T, C1, C2, p_add)
    full = H.matmul(H.arr(np.eye(w + p)) - H.matmul(H.matmul(U, T.T), (U * phi[:, None]).T), np.vstack([C1, C2]))
    assert _relerr(np.vstack([A1, A2]), full) <= 1000 * H.EPS_LD
    # on [R ; B] itself it gives [R' ; 0]
    A1, A2 = H.tp_apply(V, T, R, B, p_add)
    kappa = np.linalg.cond(np.asarray(Rn, dtype=np.float64))
    assert _relerr(A1, Rn) <= 1000 * H.EPS_LD * kappa and float(H.norm(A2)) <= 1000 * H.EPS_LD * kappa * float(H.norm(B))


def test_tp_panel_zero_column_and_lost_definiteness():
    R, B = _panel_inputs(7, 65)
    Bz = B.copy()
    Bz[:, 0] = 0.0
    Rn, V, T = H.tp_panel(R, Bz)
    assert not np.any(V[:, 0] != 0) and not np.any(T[:, 0] != 0) and np.array_equal(np.asarray(Rn[0], dtype=np.float64), R[0])
    Rs, Bs = _signed_inputs(7, 65, 64)
    bad = Bs.copy()
    bad[64] = 40.0 * Rs[2]                     # a row that was never in R, larger than everything R holds in column 2
    with pytest.raises(ArithmeticError) as ei:
        H.tp_panel(Rs, bad, 64)
    assert 0 <= ei.value.args[1] <= 2
    # trans = 0 undoes trans = 1 in the unsigned instance
    _, V, T = H.tp_panel(R, B)
    C1, C2 = H.tp_apply(V, T, R, B, trans=1)
    D1, D2 = H.tp_apply(V, T, C1, C2, trans=0)
    assert _relerr(D1, R) <= 1000 * H.EPS_LD and _relerr(D2, B) <= 1000 * H.EPS_LD
    # what lies below T's diagonal is not read
    Tn = np.asarray(T, dtype=np.float64) + np.tril(np.full((7, 7), np.nan), -1)
    E1, _ = H.tp_apply(np.asarray(V, dtype=np.float64), Tn, R, B, dtype=np.float64)
    assert np.all(np.isfinite(E1))


@pytest.mark.parametrize("r,k,wp", [(1, 1, None), (17, 7, None), (40, 32, None), (70, 64, None), (64, 36, 32), (64, 36, 4), (20, 40, None)])
def test_jacobi_pair_orthogonal_and_converged(r, k, wp):
    G = np.random.default_rng(10 * r + k).standard_normal((r, k))
    tol = np.sqrt(r) * EPS
    off, GJ, J = H.jacobi_pair(G, tol, wp=wp)
    I = H.arr(np.eye(k))
    orth = float(H.norm(H.matmul(J.T, J) - I))
    after = float(H.pair_measure(GJ)) if r >= k else None
    print(f"jacobi_pair {r}x{k}: measure {float(off):.2e} -> {after}, |J^T J - I| {orth / H.EPS_LD:.1f} eps_ld")
    assert float(off) == float(H.pair_measure(G))
    assert orth <= 1000 * H.EPS_LD
    assert _relerr(GJ, H.matmul(G, J)) <= 100 * H.EPS_LD
    if r >= k:
        assert after <= tol
    # the float64 instance: the same operation at float64 round-off
    o64, G64, J64 = H.jacobi_pair(G, tol, np.float64, wp=wp)
    assert J64.dtype == np.float64 and abs(o64 - float(off)) <= 64 * EPS * float(off)
    assert np.linalg.norm(J64.T @ J64 - np.eye(k)) <= 20 * 64 * EPS
    # at or below tol nothing happens
    off2, G2, J2 = H.jacobi_pair(np.asarray(GJ, dtype=np.float64), max(tol, 2 * float(H.pair_measure(np.asarray(GJ, dtype=np.float64)))))
    assert np.array_equal(np.asarray(J2, dtype=np.float64), np.eye(k)) and np.array_equal(np.asarray(G2, dtype=np.float64), np.asarray(GJ, dtype=np.float64))


def test_js_inner_pair_is_a_round_robin():
    seen = set()
    for st in range(63):
        step = [H.js_inner_pair(st, k) for k in range(32)]
        assert sorted(x for pr in step for x in pr) == list(range(64))
        seen.update(step)
    assert len(seen) == 64 * 63 // 2 and all(i < j for i, j in seen)
