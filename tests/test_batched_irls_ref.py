"""CPU-side checks of the restatement that the batched robust least-squares tests measure the kernels against (batched_irls_ref.py;
mi355x_qr.h section 8j): the margin that lets the GPU test ask for the restatement's solve counts with no exception, the recovery of the
planted outliers, the rank rule of the median, and the pieces the restatement is made of."""
from fractions import Fraction

import numpy as np
import pytest

import batched_irls_ref as R
import hp_ref as H


@pytest.mark.parametrize("m,n", R.SHAPES)
def test_no_deciding_change_lies_within_one_percent_of_tol(qr, m, n):
    assert bool(qr.lib.qrd_ir_wave_route(m, n)) == ((m, n) in R.WAVE_SHAPES)
    assert m <= qr.irls_batched_max_rows(n)
    for loss in R.losses(m, n):
        c = R.case(m, n, loss)
        for q, o in enumerate(c["out64"]):
            assert o["info"] == 0 and 1 <= o["iter"] <= 50 and o["status"] in (0, 2, 3)
            assert o["status"] != 3 or o["iter"] == 50
            for ch in o["changes"]:
                assert not (0.99 * R.TOL <= ch <= 1.01 * R.TOL), (m, n, R.LOSS_NAMES[loss], q, ch / R.TOL, "move this case's salt")
            # the longdouble instance, run for the same number of solves, takes the same decisions up to there (1 x 1: its residual is
            # an exact zero, the float64 instance's the rounding error of one division)
            assert m == n or [ch <= R.TOL for ch in c["outld"][q]["changes"]] == [ch <= R.TOL for ch in o["changes"]]


def test_bisquare_is_run_where_m_is_at_least_2n():
    assert [s for s in R.SHAPES if R.BISQUARE not in R.losses(*s)] == [(1, 1), (3, 2), (40, 32)]
    assert [s for s in R.SHAPES if R.recovers(*s)] == [(64, 7), (64, 15), (65, 15), (100, 20), (256, 40), (R.MAX_ROWS_63, 63)]
    assert R.max_rows(63) == R.MAX_ROWS_63


@pytest.mark.parametrize("m,n", [s for s in R.SHAPES if R.recovers(*s)])
def test_planted_outliers_are_found_and_the_fit_recovers(m, n):
    for loss in R.losses(m, n):
        c = R.case(m, n, loss)
        for q in range(R.BATCH):
            A, b, xs, rows = c["A"][q], c["b"][q], c["xstar"][q], c["rows"][q]
            assert len(rows) == R.planted_count(m, n) > 0
            o = c["out64"][q]
            ls = R.irls(A, b, R.LS)
            ratio = R.scaled_error(A, o["x"], xs) / R.scaled_error(A, ls["x"], xs)
            assert ratio < 0.5, (m, n, R.LOSS_NAMES[loss], q, ratio)
            if loss == R.HUBER:
                assert np.all(o["w"][rows] < 0.5), (m, n, q, o["w"][rows])
            else:
                assert np.all(o["w"][rows] == 0.0), (m, n, q, o["w"][rows])


def test_numpy_median_equals_the_rank_rule_ties_included():
    rng = np.random.default_rng(5)
    for cnt in list(range(1, 20)) + [63, 64, 289, 290]:
        v = np.abs(rng.standard_normal(cnt))
        assert R.median_by_ranks(v) == np.median(v)
        t = np.round(v * 4) / 4                               # many ties, zeros among them
        assert R.median_by_ranks(t) == np.median(t)
        assert R.median_by_ranks(np.full(cnt, 0.375)) == 0.375
    assert R.median_by_ranks(np.array([3.0, 1.0, 1.0, 3.0])) == 2.0 and R.median_by_ranks(np.array([0.0, 0.0, 5.0])) == 0.0
    assert np.isnan(R.median_by_ranks(np.array([1.0, np.nan, 2.0]))) and np.isnan(R.median_by_ranks(np.zeros(0)))


def test_fma64_rounds_once():
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal(2000), rng.standard_normal(2000)
    c = -a * b + rng.standard_normal(2000) * np.ldexp(1.0, rng.integers(-60, 3, 2000))      # heavy cancellation
    got = R.fma64(a, b, c)
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    x = 1.5 / 7.0
    assert R.fma64(-7.0, x, 1.5) == float(Fraction(1.5) - Fraction(7.0) * Fraction(x)) != 0.0
    assert R.fma64(-2.0, 1.5, 3.0) == 0.0


def test_least_squares_loss_is_hp_ref_lstsq_on_the_scaled_rows():
    rng = np.random.default_rng(7)
    A, b = rng.standard_normal((20, 6)), rng.standard_normal(20)
    p = rng.uniform(0.5, 2.0, 20)
    p[[3, 11]] = 0.0
    for dtype in (np.float64, H.LD):
        o = R.irls(A, b, R.LS, prior=p, dtype=dtype)
        keep = p > 0
        x, _ = H.lstsq(np.sqrt(H.arr(p[keep], dtype))[:, None] * H.arr(A[keep], dtype), np.sqrt(H.arr(p[keep], dtype)) * H.arr(b[keep], dtype), dtype)
        assert o["info"] == 0 and o["iter"] == 1 and o["status"] == 0 and np.all(o["w"] == 1)
        assert float(H.norm(H.arr(o["x"]) - H.arr(x)) / H.norm(x)) < 1e-13
    An = A.copy()
    An[3] = np.nan
    assert np.array_equal(R.irls(An, b, R.LS, prior=p)["x"], R.irls(A, b, R.LS, prior=p)["x"]), "a masked row is zeros whatever it holds"


def test_info_words_and_statuses_of_the_restatement():
    rng = np.random.default_rng(8)
    A, b = rng.standard_normal((12, 3)), rng.standard_normal(12)
    for bad in (-1.0, np.nan, np.inf):
        p = np.ones(12)
        p[5] = bad
        assert R.irls(A, b, R.HUBER, prior=p)["info"] == -1
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert R.irls(A, b, R.HUBER, scale=bad)["info"] == -1
    p = np.zeros(12)
    p[:2] = 1.0
    assert R.irls(A, b, R.HUBER, prior=p)["info"] == -2
    assert R.irls(A, b, R.BISQUARE, x0=np.zeros(3), scale=1e-9)["info"] == -2
    Az = A.copy()
    Az[:, 1] = 0.0
    assert R.irls(Az, b, R.HUBER)["info"] == 2
    o = R.irls(np.array([[2.0]]), np.array([3.0]), R.HUBER)
    assert (o["status"], o["iter"], o["x"][0], o["s"]) == (2, 1, 1.5, 0.0)
    o = R.irls(A, np.zeros(12), R.BISQUARE)
    assert o["status"] == 2 and o["iter"] == 1 and np.all(o["x"] == 0) and np.all(o["w"] == 1)
    o = R.irls(A, b, R.HUBER, maxit=1)
    assert o["status"] == 3 and o["iter"] == 1 and o["s"] > 0
    full = R.irls(A, b, R.HUBER, tol=1e-10)
    warm = R.irls(A, b, R.HUBER, tol=1e-6, x0=full["x"])
    assert full["status"] == 0 and warm["status"] == 0 and warm["iter"] == 1
