"""The restatement of the dual active-set loop that the batched inequality-constrained tests measure against
(tests/batched_lsei_ref.py): on the planted inputs of the GPU file it finds the planted set and info 0 within every cap and within maxit
candidates; against scipy's SLSQP on small random members; and the special cases of the header's section 8l.  No GPU."""
import numpy as np
import pytest

import batched_lsei_ref as R

EPS = R.EPS


@pytest.mark.parametrize("m,n,mg,neq", R.SHAPES)
def test_restatement_finds_the_planted_set_within_every_cap(m, n, mg, neq):
    c = R.case(m, n, mg, neq)
    for q in range(R.BATCH):
        o = c["out64"][q]
        assert o["info"] == 0, q
        assert np.array_equal(o["state"], c["state"][q]), q
        mu = np.asarray(o["mu"], dtype=np.float64)
        assert np.all(mu[neq:][o["state"][neq:] == 1] > 0) and np.all(mu[o["state"] == 0] == 0.0)
        assert 1 <= o["iter"] <= 3 * mg + 1, (q, o["iter"])
        for k, name in enumerate(R.NAMES):
            assert c["ref"][q][k] <= 0.5 * c["caps"][k], (q, name, c["ref"][q][k], c["caps"][k])
        scale = np.abs(c["mustar"][q]).max() if mg else 1.0
        kappa = np.linalg.cond(c["A"][q] / np.linalg.norm(c["A"][q], axis=0)[None, :])
        assert np.max(np.abs(mu - c["mustar"][q])) <= 1e4 * kappa * kappa * EPS * max(scale, 1.0) * (m + n), q


def _random_member(seed, m, n, mg, neq):
    rng = np.random.default_rng(seed)
    A, b, G = rng.standard_normal((m, n)), rng.standard_normal(m), rng.standard_normal((mg, n))
    x0 = rng.standard_normal(n)
    h = G @ x0 - np.concatenate([np.zeros(neq), rng.uniform(0.0, 1.0, mg - neq)])         # x0 is feasible
    return A, b, G, h


@pytest.mark.parametrize("seed,m,n,mg,neq", [(1, 6, 3, 4, 0), (2, 8, 4, 6, 1), (3, 10, 5, 9, 0), (4, 12, 6, 7, 2), (5, 9, 4, 12, 0),
                                              (6, 5, 5, 8, 1)])
def test_against_scipy_slsqp(seed, m, n, mg, neq):
    opt = pytest.importorskip("scipy.optimize")
    A, b, G, h = _random_member(seed, m, n, mg, neq)
    o = R.lsei(A, b, G, h, neq)
    assert o["info"] == 0
    x = np.asarray(o["x"], dtype=np.float64)
    cons = [{"type": "ineq", "fun": lambda v: G[neq:] @ v - h[neq:], "jac": lambda v: G[neq:]}]
    if neq:
        cons.append({"type": "eq", "fun": lambda v: G[:neq] @ v - h[:neq], "jac": lambda v: G[:neq]})
    res = opt.minimize(lambda v: 0.5 * np.sum((A @ v - b) ** 2), np.linalg.lstsq(G, h, rcond=None)[0], jac=lambda v: A.T @ (A @ v - b),
                       constraints=cons, method="SLSQP", options=dict(ftol=1e-12, maxiter=500))
    assert res.status in (0, 8), res.message                 # (8: the line search finds nothing to gain at the optimum)
    assert np.linalg.norm(x - res.x) <= 1e-6 * max(1.0, np.linalg.norm(x)), (x, res.x)
    got = R.measures(A, b, G, h, x, o["mu"], o["s"], o["resid"], o["state"])
    for k in range(4):
        assert got[k] <= R.caps(m, n, mg)[k], (R.NAMES[k], got[k])


def test_dependent_but_feasible_member_takes_three_candidates():
    G, h = R.DEPENDENT_FEASIBLE
    o = R.lsei(np.eye(2), np.zeros(2), G, h, 0)
    assert o["info"] == 0 and o["iter"] == 3
    assert np.array_equal(o["x"], [1.0, 0.5]) and np.array_equal(o["state"], [1, 0, 1, 0]) and np.array_equal(o["s"], [0.0, 1.0, 0.0, 0.0])


def test_infeasible_member_gives_minus_two():
    G, h = R.INFEASIBLE
    o = R.lsei(np.eye(2), np.zeros(2), G, h, 0)
    assert o["info"] == -2 and o["x"] is None and o["mu"] is None


def test_a_violated_row_that_depends_on_the_set_replaces_its_row():
    o = R.lsei(np.eye(2), np.zeros(2), np.array([[2.0, 0.0], [1.0, 0.0]]), np.array([1.0, 1.0]), 0)
    assert o["info"] == 0 and o["iter"] == 4 and np.array_equal(o["state"], [0, 1]) and o["x"][0] == 1.0 and o["mu"][1] == 1.0


def test_zero_rows_of_G():
    rng = np.random.default_rng(8)
    A, b = rng.standard_normal((6, 3)), rng.standard_normal(6)
    G, h = np.zeros((2, 3)), np.array([-1.0, 0.0])
    o = R.lsei(A, b, G, h, 0)
    assert o["info"] == 0 and o["iter"] == 1 and np.all(o["state"] == 0)
    assert R.lsei(A, b, G, np.array([-1.0, 0.5]), 0)["info"] == -2


def test_dependent_equalities_and_a_zero_column_of_A():
    rng = np.random.default_rng(9)
    A, b = rng.standard_normal((6, 3)), rng.standard_normal(6)
    G = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert R.lsei(A, b, G, np.zeros(3), 2)["info"] == -3
    A0 = A.copy()
    A0[:, 1] = 0.0
    assert R.lsei(A0, b, G[[0, 2]], np.array([-5.0, -5.0]), 0)["info"] == 2


def test_all_equalities_is_the_null_space_solve():
    import batched_lse_ref as L
    rng = np.random.default_rng(10)
    A, b, G, h = rng.standard_normal((9, 5)), rng.standard_normal(9), rng.standard_normal((3, 5)), rng.standard_normal(3)
    o = R.lsei(A, b, G, h, 3)
    X, lam, resid = L.gglse(A, G, b[:, None], h[:, None], np.float64)
    assert o["info"] == 0 and o["iter"] == 1 and np.array_equal(o["x"], X[:, 0]) and np.array_equal(o["mu"], -lam[:, 0])


def test_maxit_two_returns_the_last_accepted_pair_with_info_n_plus_one():
    c = R.case(16, 7, 20, 2)
    hit = 0
    for q in range(R.BATCH):
        full = c["out64"][q]
        o = R.lsei(c["A"][q], c["b"][q], c["G"][q], c["h"][q], 2, maxit=2)
        if full["iter"] > 2:
            hit += 1
            assert o["info"] == 8 and o["iter"] == 2
            assert np.min(o["s"][2:]) < 0                                                  # s shows what the pair still violates
            got = R.measures(c["A"][q], c["b"][q], c["G"][q], c["h"][q], o["x"], o["mu"], o["s"], o["resid"], np.zeros(20, dtype=int))
            assert got[1] <= c["caps"][1] and got[2] <= c["caps"][2]                       # the pair is a stationary one
    assert hit >= 5


def test_restatement_is_exactly_homogeneous():
    """(A, b) x 2^a and (G, h) x 2^c: the same x, state and count, mu x 2^(2a - c), resid x 2^a, s x 2^c -- what the GPU file asserts of the
    kernels holds of the restatement"""
    c = R.case(16, 15, 15, 0)
    A, b, G, h = (c[k][1] for k in ("A", "b", "G", "h"))
    o = c["out64"][1]
    for ea, ec in ((20, 0), (0, -11), (6, -7)):
        sa, sc = 2.0 ** ea, 2.0 ** ec
        o2 = R.lsei(sa * A, sa * b, sc * G, sc * h, 0)
        assert np.array_equal(o2["x"], o["x"]) and np.array_equal(o2["state"], o["state"]) and o2["iter"] == o["iter"]
        assert np.array_equal(o2["mu"], (sa * sa / sc) * o["mu"]) and o2["resid"] == sa * o["resid"] and np.array_equal(o2["s"], sc * o["s"])
