"""The reference of the batched trust-region step (tests/batched_trust_ref.py) checked without a device: the float64 restatement meets
the termination rule on every named input, its |D x| re-evaluated in longdouble from the stacked system of the lambda it found stays
within rtol Delta plus the damped call's xnorm cap, and no member runs out of iterations."""
import numpy as np
import pytest

import batched_damped_ref as D
import batched_trust_ref as T
import hp_ref as H

# (m, n, members): the orders of the GPU test on members small enough for a longdouble truth of every one
CASES = [(1, 1, 5), (5, 3, 5), (17, 15, 5), (19, 17, 5), (33, 31, 5), (35, 33, 5), (65, 63, 3)]


@pytest.mark.parametrize("rtol", T.RTOLS)
@pytest.mark.parametrize("m,n,count", CASES)
def test_float64_restatement_meets_the_rule_and_the_truth(m, n, count, rtol):
    A, b, d = T.batch(m, n, count)
    worst_it = 0
    for q in range(count):
        R, z, rss = T.factors(A[q], b[q])
        delta = T.FRACS[q % len(T.FRACS)] * T.gauss_newton_dxnorm(R, z, d[q])
        r = T.lmpar(R, z, delta, d[q], rss=rss, rtol=rtol)
        assert r["info"] == 0 and r["status"] in (0, 1), (q, r["status"])
        assert r["iter"] <= T.MAXIT and (r["status"] == 1) == (r["iter"] == 0) == (r["lam"] == 0)
        if T.FRACS[q % len(T.FRACS)] >= 1.05:
            assert r["status"] == 1
        assert T.meets_rule(r["xnorm"], r["lam"], delta, rtol), (q, r["xnorm"], delta)
        worst_it = max(worst_it, r["iter"])
        # the truth: |D x(lambda)| of the stacked system in longdouble
        if r["lam"] == 0 and m == n:
            continue                                       # a square member at lambda = 0 has no least-squares truth of its own
        tr = D.truth(A[q], b[q][:, None], r["lam"], d[q])
        cap = D.caps(A[q], b[q][:, None], r["lam"], d[q], tr)[1]
        xn = float(tr[1][0])
        slack = rtol * delta + cap * xn
        if r["lam"] == 0:
            assert xn <= delta + slack, (q, xn, delta)
        else:
            assert abs(xn - delta) <= slack, (q, xn, delta)
        assert abs(float(r["resid"]) - float(tr[2][0])) <= D.caps(A[q], b[q][:, None], r["lam"], d[q], tr)[2] * float(tr[2][0])
    print(f"{m}x{n} rtol {rtol}: at most {worst_it} iterations")


def test_restatement_agrees_with_its_longdouble_instance():
    A, b, d = T.batch(12, 7, 5)
    for q in range(5):
        R, z, rss = T.factors(A[q], b[q])
        delta = 0.3 * T.gauss_newton_dxnorm(R, z, d[q])
        r64 = T.lmpar(R, z, delta, d[q], rss=rss, rtol=1e-3)
        rld = T.lmpar(R, z, delta, d[q], rss=rss, rtol=1e-3, dtype=H.LD)
        assert r64["iter"] == rld["iter"] and r64["status"] == rld["status"] == 0
        assert abs(float(r64["lam"]) - float(rld["lam"])) <= 1e-9 * float(rld["lam"])


def test_rank_deficient_and_invalid_members():
    A, b, d = T.batch(9, 6, 4)
    for q in range(4):
        R, z, rss = T.factors(A[q], b[q])
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert T.lmpar(R, z, bad, d[q])["info"] == -1
        R[:, 4:] = 0.0                                     # exactly zero trailing columns: nsing = 4
        full = T.gauss_newton_dxnorm(R[:4, :4], z[:4], d[q][:4])
        for f in (2.0, 0.5, 1e-3):
            r = T.lmpar(R, z, f * full, d[q], rss=rss)
            assert r["info"] == 0 and r["status"] in (0, 1, 2)
            assert r["xnorm"] <= 1.1 * f * full
        dz = d[q].copy()
        dz[4] = 0.0                                        # nothing damps the zero column: the elimination leaves a zero on the diagonal
        assert T.lmpar(R, z, 0.5 * full, dz, rss=rss)["info"] == 5


def test_warm_start_and_pivoted_order():
    A, b, d = T.batch(20, 9, 3)
    for q in range(3):
        R, z, rss = T.factors(A[q], b[q])
        delta = 0.2 * T.gauss_newton_dxnorm(R, z, d[q])
        cold = T.lmpar(R, z, delta, d[q], rss=rss, rtol=1e-3)
        warm = T.lmpar(R, z, delta, d[q], rss=rss, rtol=1e-3, lam0=cold["lam"])
        assert warm["iter"] <= cold["iter"] and warm["iter"] == 1 and T.meets_rule(warm["xnorm"], warm["lam"], delta, 1e-3)
        # the factors of A P with the columns reversed: the same problem, X in the caller's order
        jp = np.arange(9)[::-1].copy()
        Rp, zp, rssp = T.factors(A[q][:, jp], b[q])
        piv = T.lmpar(Rp, zp, delta, d[q], jpvt=jp, rss=rssp, rtol=1e-3)
        assert piv["status"] == 0 and np.allclose(piv["X"], cold["X"], rtol=1e-2, atol=0)
