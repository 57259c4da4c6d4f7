"""The restatement of the null-space method that the batched constrained least-squares tests measure against (tests/batched_lse_ref.py):
its float64 instance against its longdouble instance, against LAPACK dgglse where scipy imports, the multipliers against the KKT identity,
and the two edges p == n and m == n - p.  No GPU."""
import numpy as np
import pytest

import batched_lse_ref as R
import hp_ref as H

EPS = R.EPS


@pytest.mark.parametrize("m,n,p,nrhs", R.SHAPES)
def test_float64_instance_stays_within_the_caps(m, n, p, nrhs):
    """every measure of the float64 instance is under half its cap on every input of the GPU file (the tiny shapes, whose caps are a few
    eps, are what keeps this from being a quarter): four times the reference, capped, is a bound the kernels can be held to"""
    c = R.case(m, n, p, nrhs)
    for q in range(R.BATCH):
        for j in range(nrhs):
            for k, name in enumerate(R.NAMES):
                assert c["ref"][q][j][k] <= 0.5 * c["caps"][q][j][k], (q, j, name, c["ref"][q][j][k], c["caps"][q][j][k])


@pytest.mark.parametrize("m,n,p,nrhs", R.SHAPES)
def test_longdouble_instance_satisfies_constraint_and_kkt(m, n, p, nrhs):
    """the reference itself: C x = d and A^T (A x - b) + C^T lam = 0 to a few eps of longdouble times the conditioning, resid = ||A x - b||"""
    c = R.case(m, n, p, nrhs)
    for q in range(R.BATCH):
        got = R.measures(c["A"][q], c["C"][q], c["B"][q], c["D"][q], c["Xld"][q], c["lamld"][q], c["residld"][q], c["Xld"][q])
        for j in range(nrhs):
            assert got[j][0] <= (n + 8) * H.EPS_LD and got[j][1] <= (n + 8) * H.EPS_LD and got[j][2] <= (m + n) * H.EPS_LD, (q, j, got[j])


@pytest.mark.parametrize("m,n,p,nrhs", R.SHAPES)
def test_against_lapack_dgglse(m, n, p, nrhs):
    lapack = pytest.importorskip("scipy.linalg.lapack")
    c = R.case(m, n, p, nrhs)
    for q in range(R.BATCH):
        for j in range(nrhs):
            out = lapack.dgglse(c["A"][q], c["C"][q], c["B"][q][:, j], c["D"][q][:, j])
            x, info = out[3], out[4]              # (t, r, res, x, info): at n == 1 several of them have x's shape
            assert info == 0
            xl = np.asarray(c["Xld"][q][:, j], dtype=np.float64)
            assert np.linalg.norm(x - xl) <= c["caps"][q][j][3] * np.linalg.norm(xl), (q, j)


def test_p_equals_n_fixes_x_by_the_constraints():
    c = R.case(8, 5, 5, 2)
    for q in range(R.BATCH):
        x = np.linalg.solve(c["C"][q], c["D"][q])
        xl = np.asarray(c["Xld"][q], dtype=np.float64)
        assert np.linalg.norm(x - xl) <= 50 * np.linalg.cond(c["C"][q]) * EPS * np.linalg.norm(xl)
        r = np.linalg.norm(c["A"][q] @ xl - c["B"][q], axis=0)
        assert np.allclose(np.asarray(c["residld"][q], dtype=np.float64), r, rtol=1e-12)


def test_m_equals_n_minus_p_leaves_an_exact_zero_residual():
    c = R.case(1, 2, 1, 1)
    for q in range(R.BATCH):
        assert float(c["residld"][q][0]) == 0.0
        X6, l6, r6 = R.gglse(c["A"][q], c["C"][q], c["B"][q], c["D"][q], np.float64)
        assert r6[0] == 0.0 and np.all(l6 == 0.0)             # nothing left over: the multipliers vanish with the residual
        M = np.vstack([c["A"][q], c["C"][q]])
        x = np.linalg.solve(M, np.concatenate([c["B"][q], c["D"][q]]))
        assert np.allclose(X6, x, rtol=1e-9)


def test_instances_are_exactly_homogeneous_in_the_right_hand_sides():
    """scaling (b, d) by a power of two scales X, lam and resid exactly: what the GPU file asserts of the kernels holds of the reference"""
    c = R.case(16, 8, 3, 1)
    A, C, B, D = c["A"][0], c["C"][0], c["B"][0], c["D"][0]
    X, lam, res = R.gglse(A, C, B, D, np.float64)
    X2, lam2, res2 = R.gglse(A, C, 8.0 * B, 8.0 * D, np.float64)
    assert np.array_equal(X2, 8.0 * X) and np.array_equal(lam2, 8.0 * lam) and np.array_equal(res2, 8.0 * res)
