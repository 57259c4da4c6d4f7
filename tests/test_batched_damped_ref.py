"""The reference of the batched damped least squares (tests/batched_damped_ref.py) checked without a device: against the closed form at
benign conditioning, the flip identity of the wide case, pivoted factors, and that the float64 instance of the two-stage restatement
stays inside the caps on every case tests/test_gpu_batched_damped.py uses."""
import numpy as np
import pytest

import batched_damped_ref as D
import hp_ref as H

EPS = D.EPS


def _closed_form(A, B, lam, d):
    n = A.shape[1]
    dd = np.ones(n) if d is None else d
    return np.linalg.solve(A.T @ A + lam ** 2 * np.diag(dd ** 2), A.T @ B)


@pytest.mark.parametrize("m,n,nrhs", [(5, 3, 2), (20, 8, 1), (40, 17, 3)])
@pytest.mark.parametrize("dtype", [np.float64, D.LD])
def test_two_stage_restatement_equals_the_closed_form(m, n, nrhs, dtype):
    A, B = D.U(m * n, m, n), D.U(m * n + 1, m, nrhs)
    d = 0.5 + 1.5 * np.random.default_rng(7).random(n)
    a2 = np.linalg.norm(A, 2)
    lams = [0.0, 0.3 * a2, 30 * a2]
    for dd in (None, d):
        out = D.tall(A, B, lams, dd, dtype)
        for lam, (X, xn, rs, info) in zip(lams, out):
            Xc = _closed_form(A, B, lam, dd)
            X = np.asarray(X, dtype=np.float64)
            kappa = np.linalg.cond(A) ** 2
            assert info == 0 and np.linalg.norm(X - Xc) <= 50 * kappa * EPS * np.linalg.norm(Xc)
            w = np.ones(n) if dd is None else dd
            assert np.allclose(np.asarray(xn, dtype=np.float64), np.linalg.norm(w[:, None] * Xc, axis=0), rtol=1e-10)
            assert np.allclose(np.asarray(rs, dtype=np.float64), np.linalg.norm(A @ Xc - B, axis=0), rtol=1e-10)


def test_the_truth_is_the_closed_form():
    A, B = D.U(3, 12, 5), D.U(4, 12, 2)
    d = np.linspace(0.5, 2.0, 5)
    X, xn, rs = D.truth(A, B, 0.7, d)
    Xc = _closed_form(A, B, 0.7, d)
    assert np.linalg.norm(np.asarray(X, dtype=np.float64) - Xc) <= 1e-13 * np.linalg.norm(Xc)


@pytest.mark.parametrize("m,n", [(6, 7), (3, 31), (33, 100)])
def test_flip_identity_solves_the_wide_system(m, n):
    A, B = D.U(m + n, m, n), D.U(m + n + 1, m, 2)
    a2 = np.linalg.norm(A, 2)
    lams = [1e-8 * a2, 0.3 * a2, 30 * a2]
    out = D.wide(A, B, lams)
    for lam, (X, xn, rs, info) in zip(lams, out):
        S = np.vstack([A, lam * np.eye(n)])
        C = np.vstack([B, np.zeros((n, 2))])
        Xn = np.linalg.lstsq(S, C, rcond=None)[0]
        kappa = np.linalg.cond(S)
        bound = kappa + kappa ** 2 * np.linalg.norm(S @ Xn - C) / (np.linalg.norm(S, 2) * np.linalg.norm(Xn))
        assert info == 0 and np.linalg.norm(X - Xn) <= 50 * bound * EPS * np.linalg.norm(Xn)
        assert np.allclose(xn, np.linalg.norm(Xn, axis=0), rtol=1e-9)
        assert np.allclose(rs, np.linalg.norm(A @ Xn - B, axis=0), rtol=1e-6, atol=1e-12 * a2)


def test_pivoted_factors_give_the_solution_in_the_callers_order():
    A, B = D.U(11, 30, 9), D.U(12, 30, 2)
    d = 0.5 + 1.5 * np.random.default_rng(5).random(9)
    F, tau, jp = H.qrp(A, np.float64)
    QtB = H.apply_q(F, tau, B, "T", np.float64)
    lam = 0.3 * np.linalg.norm(A, 2)
    X, xn, rs, info = D.solve(H.triu(F), QtB[:9], lam, d, jp, (QtB[9:] ** 2).sum(axis=0))
    Xc = _closed_form(A, B, lam, d)
    assert info == 0 and np.linalg.norm(X - Xc) <= 1e-12 * np.linalg.norm(Xc)
    assert np.allclose(rs, np.linalg.norm(A @ Xc - B, axis=0), rtol=1e-10)


def test_a_zero_diagonal_is_reported_and_nothing_is_returned():
    R = np.triu(D.U(2, 4, 4))
    R[:, 2] = 0.0
    Z = D.U(3, 4, 1)
    assert D.solve(R, Z, 0.0)[3] == 3
    assert D.solve(R, Z, 0.5, np.array([1.0, 1.0, 0.0, 1.0]))[3] == 3
    assert D.solve(R, Z, 0.5)[3] == 0
    X, _, _, info = D.solve(np.zeros((3, 3)), np.zeros((3, 2)), 0.25)          # an empty accumulator
    assert info == 0 and np.all(X == 0)


def _inside(c):
    worst = 0.0
    for rq, cq in zip(c["ref"], c["caps"]):
        for r, cp in zip(rq, cq):
            for k in range(4):
                assert np.isfinite(r[k]) and r[k] <= cp[k], (D.NAMES[k], r[k], cp[k])
                worst = max(worst, r[k] / cp[k])
    return worst


@pytest.mark.parametrize("m,n,nrhs", D.SHAPES)
def test_float64_instance_stays_inside_the_caps_tall(m, n, nrhs):
    """the caps are reachable by the restatement in working precision: the worst ratio is printed (-s)"""
    for with_d in (True, False) if (m, n) == (64, 28) else (True,):
        print(f"{m}x{n} nrhs={nrhs} d={with_d}: worst measure / cap = {_inside(D.case(m, n, nrhs, with_d)):.4f}")


@pytest.mark.parametrize("rows,cols", D.WIDE)
def test_float64_instance_stays_inside_the_caps_wide(rows, cols):
    for nrhs in D.WIDE_NRHS:
        print(f"wide {cols}x{rows} nrhs={nrhs}: worst measure / cap = {_inside(D.case(cols, rows, nrhs, False, 5)):.4f}")
