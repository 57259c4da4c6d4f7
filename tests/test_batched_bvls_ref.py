"""The restatement of bounded-variable least squares that the batched bound-constrained tests measure against (tests/batched_bvls_ref.py):
on the planted inputs of the GPU file it finds x*, the planted state and info 0 within 2 n + 2 eliminations; against scipy's BVLS where
scipy imports; and the special cases of the header's section 8i.  No GPU."""
import numpy as np
import pytest

import batched_bvls_ref as R

EPS = R.EPS
INF = np.inf


@pytest.mark.parametrize("m,n", R.SHAPES)
def test_restatement_finds_the_planted_solution(m, n):
    c = R.case(m, n)
    for q in range(R.BATCH):
        o = c["out64"][q]
        assert o["info"] == 0, q
        assert np.array_equal(o["state"], c["state"][q]), q
        x = np.asarray(o["x"], dtype=np.float64)
        assert np.all(x >= c["lo"][q]) and np.all(x <= c["hi"][q])                        # no tolerance
        at_lo, at_hi = o["state"] == -1, o["state"] == 1
        assert np.array_equal(x[at_lo], c["lo"][q][at_lo]) and np.array_equal(x[at_hi], c["hi"][q][at_hi])
        assert np.all(o["w"][at_lo] < 0) and np.all(o["w"][at_hi] > 0)
        assert o["iter"] <= 2 * n + 2, (q, o["iter"])
        kappa = np.linalg.cond(c["A"][q])
        assert np.linalg.norm(x - c["xstar"][q]) <= 1e3 * kappa * kappa * EPS * max(1.0, np.linalg.norm(c["xstar"][q])), q
        for k, name in enumerate(R.NAMES):
            assert c["ref"][q][k] <= 0.5 * c["cap"], (q, name, c["ref"][q][k], c["cap"])


@pytest.mark.parametrize("m,n", R.SHAPES)
def test_against_scipy_bvls(m, n):
    opt = pytest.importorskip("scipy.optimize")
    c = R.case(m, n)
    for q in range(R.BATCH):
        res = opt.lsq_linear(c["A"][q], c["b"][q], bounds=(c["lo"][q], c["hi"][q]), method="bvls", tol=1e-13)
        x = np.asarray(c["out64"][q]["x"], dtype=np.float64)
        got = R.measures(c["A"][q], c["b"][q], res.x, None, None, c["state"][q])[0]
        ours = R.measures(c["A"][q], c["b"][q], x, None, None, c["state"][q])[0]
        assert ours <= c["cap"]
        # the two solutions agree as far as the conditioning lets two backward-stable solves agree
        kappa = np.linalg.cond(c["A"][q])
        assert np.linalg.norm(x - res.x) <= 1e3 * kappa * kappa * EPS * max(1.0, np.linalg.norm(x)), (q, got, ours)


def _small(seed=3, m=12, n=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m, n)), rng.standard_normal(m)


def test_bad_bounds_give_minus_one():
    A, b = _small()
    lo, hi = -np.ones(5), np.ones(5)
    for j, (l, h) in enumerate([(1.5, 1.0), (np.nan, 1.0), (-1.0, np.nan), (INF, INF), (-INF, -INF)]):
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[j], hi2[j] = l, h
        o = R.bvls(A, b, lo2, hi2)
        assert o["info"] == -1 and o["x"] is None
    assert R.bvls(A, b, lo, hi)["info"] == 0


def test_a_fixed_variable_is_legal_and_never_freed():
    A, b = _small()
    lo, hi = -np.ones(5), np.ones(5)
    lo[2] = hi[2] = 0.25
    o = R.bvls(A, b, lo, hi)
    assert o["info"] == 0 and o["state"][2] == -1 and o["x"][2] == 0.25
    keep = [0, 1, 3, 4]
    o2 = R.bvls(A[:, keep], b - 0.25 * A[:, 2], lo[keep], hi[keep])
    assert np.allclose(np.asarray(o["x"])[keep], o2["x"], rtol=0, atol=1e-13) and np.array_equal(o["state"][keep], o2["state"])


def test_all_unbounded_takes_one_elimination():
    A, b = _small()
    for lo, hi in ((None, None), (np.full(5, -INF), np.full(5, INF))):
        o = R.bvls(A, b, lo, hi)
        assert o["info"] == 0 and o["iter"] == 1 and np.all(o["state"] == 0)
        assert np.allclose(o["x"], np.linalg.lstsq(A, b, rcond=None)[0], rtol=0, atol=1e-13)


def test_a_start_that_is_optimal_takes_no_elimination():
    A, b = _small()
    lo = np.zeros(5)
    b2 = -np.abs(b)                                                                       # A^T b < 0 wherever A > 0 and b < 0 ...
    o = R.bvls(np.abs(A), b2, lo, None)                                                   # ... so x = 0 is the NNLS solution
    assert o["info"] == 0 and o["iter"] == 0 and np.all(o["state"] == -1) and np.all(o["x"] == 0) and np.all(o["w"] < 0)


def test_an_exactly_zero_free_column_gives_its_index():
    A, b = _small()
    A = A.copy()
    A[:, 3] = 0.0
    o = R.bvls(A, b, None, None)                                                          # free from the start
    assert o["info"] == 4 and o["x"] is None
    lo, hi = np.full(5, -INF), np.full(5, INF)
    lo[3], hi[3] = -1.0, 1.0                                                              # bound at the start: w_3 == 0, never freed
    o = R.bvls(A, b, lo, hi)
    assert o["info"] == 0 and o["state"][3] == -1


def test_maxit_one_returns_a_feasible_iterate_with_info_n_plus_one():
    c = R.case(16, 7)
    hit = 0
    for q in range(R.BATCH):
        full = c["out64"][q]
        o = R.bvls(c["A"][q], c["b"][q], c["lo"][q], c["hi"][q], maxit=1)
        if full["iter"] > 1:
            hit += 1
            assert o["info"] == 8 and o["iter"] == 1
            x = np.asarray(o["x"], dtype=np.float64)
            assert np.all(x >= c["lo"][q]) and np.all(x <= c["hi"][q])
            w, resid = R.gradient(c["A"][q], c["b"][q], x)
            assert np.array_equal(w, o["w"]) and resid == o["resid"]
    assert hit >= 5


def test_restatement_is_exactly_homogeneous():
    """(A, b) x 2^20: the same x, state and count, w x 2^40, resid x 2^20; (b, lo, hi) x 2^7: x, w and resid scale exactly -- what the GPU
    file asserts of the kernels holds of the restatement"""
    c = R.case(16, 15)
    A, b, lo, hi = c["A"][1], c["b"][1], c["lo"][1], c["hi"][1]
    o = c["out64"][1]
    s = 2.0 ** 20
    o2 = R.bvls(s * A, s * b, lo, hi)
    assert np.array_equal(o2["x"], o["x"]) and np.array_equal(o2["state"], o["state"]) and o2["iter"] == o["iter"]
    assert np.array_equal(o2["w"], s * s * o["w"]) and o2["resid"] == s * o["resid"]
    s = 2.0 ** 7
    o3 = R.bvls(A, s * b, s * lo, s * hi)
    assert np.array_equal(o3["x"], s * o["x"]) and np.array_equal(o3["w"], s * o["w"]) and o3["resid"] == s * o["resid"]
    assert np.array_equal(o3["state"], o["state"]) and o3["iter"] == o["iter"]
