"""CPU-side checks of the numpy restatement of the batched Levenberg-Marquardt solver (tests/batched_lm_ref.py) against the real MINPACK
(scipy.optimize.leastsq is lmder when Dfun is given), and of the condition under which tests/test_gpu_batched_lm.py may demand equal
counts: the float64 and the longdouble instance take the same decisions on every member of every problem."""
import functools

import numpy as np
import pytest

import scipy.optimize as scipy_optimize

import batched_lm_ref as L
import batched_trust_ref as T


@functools.lru_cache(maxsize=None)
def _runs(name):
    p = L.PROBLEMS[name]
    x0, data, xs = p.members(p.batch)
    out = []
    for q in range(p.batch):
        d = None if data is None else data[q]
        out.append((L.solve(p, x0[q], d, np.float64, **p.options)[0], L.solve(p, x0[q], d, L.LD, **p.options)[0]))
    return p, x0, data, xs, out


def test_the_problem_list_is_the_one_the_gpu_tests_run():
    names = set(L.PROBLEMS)
    assert {"expdecay16", "expdecay64", "gausspeak", "rosenbrock", "powell", "square1"} <= names
    for m, n in ((5, 3), (64, 31), (65, 4), (64, 32), (100, 33), (256, 63)):
        assert f"linfull{m}x{n}" in names and f"linrank1_{m}x{n}" in names
    assert {p.batch for p in L.PROBLEMS.values()} == {9, 5, 1}
    assert (L.PROBLEMS["expdecay16"].m, L.PROBLEMS["expdecay64"].m, L.PROBLEMS["gausspeak"].m, L.PROBLEMS["gausspeak"].n) == (16, 64, 32, 4)
    assert len(L.STEP_SHAPES) == 8


@pytest.mark.parametrize("name", sorted(L.PROBLEMS))
def test_float64_restatement_and_minpack_agree(name):
    p, x0, data, xs, runs = _runs(name)
    o = dict(L.DEFAULTS)
    o.update(p.options)
    for q, (r64, _) in enumerate(runs):
        d = None if data is None else data[q]
        x, _cov, info, _msg, ier = scipy_optimize.leastsq(lambda x: p.f(np, x, d), x0[q], Dfun=lambda x: p.jac(np, x, d), full_output=True,
                                                         ftol=o["ftol"], xtol=o["xtol"], gtol=o["gtol"], factor=o["factor"])
        assert r64.info == 0 and r64.status == ier, (q, r64.status, ier)
        assert r64.nfev == info["nfev"], (q, r64.nfev, info["nfev"])
        assert np.linalg.norm(np.asarray(r64.x, dtype=np.float64) - x) <= 100 * o["xtol"] * np.linalg.norm(x), q
        if p.planted:
            assert np.linalg.norm(np.asarray(r64.x, dtype=np.float64) - xs[q]) <= 100 * o["xtol"] * np.linalg.norm(xs[q]), q


@pytest.mark.parametrize("name", sorted(L.PROBLEMS))
def test_float64_and_longdouble_take_the_same_decisions(name):
    p, x0, data, xs, runs = _runs(name)
    for q, (r64, rld) in enumerate(runs):
        assert (r64.status, r64.nfev, r64.njev, r64.iter, r64.info) == (rld.status, rld.nfev, rld.njev, rld.iter, rld.info), q


def test_rules_a_and_b_stay_within_rounding():
    """fnorm from Q^T f against |f|, acnorm from the columns of R against the columns of J: the two places where the solver is not
    MINPACK to the letter"""
    for name in ("expdecay64", "gausspeak", "linfull100x33", "powell"):
        p = L.PROBLEMS[name]
        x0, data, _ = p.members(p.batch)
        d = None if data is None else data[0]
        J, f = p.jac(np, x0[0], d), p.f(np, x0[0], d)
        mem = L.Member(x0[0], np.float64, **p.options)
        mem.step(J, f)
        m, n = J.shape
        assert abs(float(mem.fnorm) - np.linalg.norm(f)) <= 2 * (m + n) * L.EPS * np.linalg.norm(f)
        acn = np.linalg.norm(J, axis=0)
        assert np.all(np.abs(np.asarray(mem.D, dtype=np.float64) - np.where(acn == 0, 1.0, acn)) <= 2 * (m + n) * L.EPS * acn.max())


def test_search_is_the_trust_region_restatement_with_the_start_given_as_par():
    for n in (3, 17):
        A, b, d = T.member(4242 + n, n + 5, n)
        R, z, _ = T.factors(A, b)
        delta = 0.3 * T.gauss_newton_dxnorm(R, z, d)
        for lam0 in (0.0, 0.25, 2.0):
            want = T.lmpar(R, z, delta, d, lam0=lam0)
            got = L.search(R, z, delta, d, None, lam0 * lam0, 0.1, T.MAXIT)
            assert got["info"] == want["info"] == 0 and (got["iter"], got["status"]) == (want["iter"], want["status"])
            assert np.array_equal(got["X"], want["X"]) and np.sqrt(got["par"]) == want["lam"] and got["xnorm"] == want["xnorm"]


def test_update_rules_on_hand_computed_cases():
    def member(**kw):
        mem = L.Member(np.array([3.0, 4.0]), np.float64)
        mem.xtrial, mem.njev, mem.iter = np.array([6.0, 8.0]), 1, 1
        mem.fnorm, mem.xnorm, mem.prered, mem.dirder, mem.par, mem.delta, mem.pnorm, mem.gnorm = 1.0, 5.0, 0.5, -0.4, 0.25, 2.0, 1.5, 0.5
        for k, v in kw.items():
            setattr(mem, k, v)
        return mem

    mem = member()
    mem.update(np.array([0.5, 0.0]))                      # actred 0.75, ratio 1.5: the radius doubles the step, par halves, accepted
    assert (mem.delta, mem.par, mem.accepted, mem.iter, mem.nfev, mem.status) == (3.0, 0.125, 1, 2, 2, 0)
    assert np.array_equal(mem.x, [6.0, 8.0]) and mem.xnorm == 10.0 and mem.fnorm == 0.5
    mem = member()
    mem.update(np.array([20.0, 0.0]))                     # ten times worse: actred -1, the 0.1 floor, rejected
    assert (mem.delta, mem.par, mem.accepted, mem.iter, mem.status) == (0.1 * 2.0, 0.25 / 0.1, 0, 1, 0) and np.array_equal(mem.x, [3.0, 4.0])
    mem = member()
    mem.update(np.array([np.nan, 0.0]))                   # not finite: as ten times worse
    assert (mem.delta, mem.par, mem.accepted, mem.status) == (0.1 * 2.0, 0.25 / 0.1, 0, 0)
    mem = member(delta=1e-9, pnorm=1e-9, prered=0.8)
    mem.update(np.array([0.8, 0.0]))                      # ratio 0.45: nothing changes, accepted, delta <= xtol |D x|
    assert (mem.delta, mem.par, mem.accepted, mem.status) == (1e-9, 0.25, 1, 2)
    mem = member(nfev=L.Member(np.zeros(2)).o["maxfev"] - 1, prered=0.8)
    mem.update(np.array([0.8, 0.0]))
    assert mem.status == 5
