"""The numpy restatement of the batched covariance, standard errors and leverages (batched_stats_ref.py) against itself, without a GPU:
its float64 instance stays inside the caps that tests/test_gpu_batched_stats.py applies to the kernels, on that file's shapes and seeds;
the longdouble instance satisfies the identities of a hat matrix and of an inverse; the rank-deficient scatter leaves exact zeros."""
import numpy as np
import pytest

import batched_stats_ref as S
import hp_ref as H

F64 = lambda v: np.asarray(v, dtype=np.float64)            # noqa: E731


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("m,n", S.FIT_SHAPES, ids=[f"{m}x{n}" for m, n in S.FIT_SHAPES])
def test_float64_restatement_stays_inside_the_caps(m, n, weighted):
    for q, (ld, f64, kap) in enumerate(S.reference_case(m, n, weighted)):
        assert ld["info"] == 0 and f64["info"] == 0, (q, ld["info"], f64["info"])
        for scaled in (False, True):
            if scaled and ld["dof"] == 0:
                continue                                   # (the scaled call refuses: info -3)
            a, b = (S.with_scale(f64), S.scaled_reference(ld, f64["sigma2"])) if scaled else (f64, ld)
            err = S.errors(a, b)
            for name in S.NAMES:
                print(f"{m}x{n} weighted={weighted} scaled={scaled} q={q} {name}: {err[name] / (kap * S.EPS):.2f} kappa eps")
                assert err[name] <= S.CAP * kap * S.EPS, (q, scaled, name, err[name] / (kap * S.EPS))
        A, bb, p = S.make_case(m, n, weighted)
        se_, ss_ = S.residual_scales(A[q], bb[q], None if p is None else p[q], ld)
        de = float(np.max(np.abs(F64(H.arr(f64["e"]) - ld["e"]))))
        print(f"{m}x{n} weighted={weighted} q={q} e: {de / (S.EPS * se_):.2f} eps nrm")
        assert de <= (m + n) * S.EPS * se_
        if ld["dof"] > 0:
            ds = abs(float(H.arr(f64["sigma2"]) - ld["sigma2"]))
            print(f"{m}x{n} weighted={weighted} q={q} sigma2: {ds / (S.EPS * ss_):.2f} eps scale")
            assert ds <= (m + n) * S.EPS * ss_
        xs = float(np.max(np.abs(F64(ld["x"])))) or 1.0
        assert np.max(np.abs(F64(f64["x"]) - F64(ld["x"]))) <= S.CAP * kap * S.EPS * xs


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("m,n", S.FIT_SHAPES, ids=[f"{m}x{n}" for m, n in S.FIT_SHAPES])
def test_reference_satisfies_the_identities(m, n, weighted):
    A, b, p = S.make_case(m, n, weighted)
    for q, (ld, _, kap) in enumerate(S.reference_case(m, n, weighted)):
        h = F64(ld["h"])
        assert abs(h.sum() - n) <= 1e-12 * n * kap
        assert h.min() >= 0.0 and h.max() <= 1.0 + 1e-12 * kap
        pq = np.ones(m) if p is None else p[q]
        assert np.all(h[pq == 0] == 0.0) and np.all(F64(ld["e"])[pq == 0] == 0.0)
        Al = H.arr(A[q])
        G = Al.T @ (H.arr(pq)[:, None] * Al)
        E = F64(ld["C"] @ G - np.eye(n))
        assert np.linalg.norm(E) <= 1e-14 * n * kap * kap, (q, np.linalg.norm(E))
        assert ld["dof"] == int((pq > 0).sum()) - n
        if ld["dof"] > 0:
            assert abs(float(ld["sigma2"]) - float((pq * F64(ld["e"]) ** 2).sum() / ld["dof"])) <= 1e-12 * float(ld["sigma2"])
        else:
            assert float(ld["sigma2"]) == np.inf


def test_info_words_of_the_restatement():
    A, b, _ = S.make_case(5, 3, False)
    assert S.fit_stats(A[0], b[0], [1, 1, -1, 1, 1])["info"] == -1
    assert S.fit_stats(A[0], b[0], [1, 1, np.nan, 1, 1])["info"] == -1 and S.fit_stats(A[0], b[0], [1, 1, np.inf, 1, 1])["info"] == -1
    assert S.fit_stats(A[0], b[0], [1, 1, 0, 0, 0])["info"] == -2
    assert S.fit_stats(A[0], b[0], [1, 1, 1, 0, 0], scaled=True)["info"] == -3
    r = S.fit_stats(A[0], b[0], [1, 1, 1, 0, 0], scaled=False)
    assert r["info"] == 0 and r["dof"] == 0 and r["sigma2"] == np.inf
    Z = A[0].copy()
    Z[:, 1] = 0.0
    assert S.fit_stats(Z, b[0])["info"] == 2


@pytest.mark.parametrize("n,rank", [(7, 0), (7, 3), (33, 20), (64, 63)])
def test_rank_deficient_scatter_leaves_zero_rows_and_columns(n, rank):
    A = S.rank_deficient_case(n, rank, 2)
    for q in range(2):
        F, _, jp = H.qrp(A[q], np.float64)
        R = H.triu(F[:n, :n])
        if rank:
            assert abs(R[rank - 1, rank - 1]) > 1e-8 * abs(R[0, 0])
        for dt in (np.float64, H.LD):
            C, se = S.covar_from_r(R, jp, rank, 2.0, dt)
            C = F64(C)
            drop = jp[rank:]
            assert np.all(C[drop, :] == 0.0) and np.all(C[:, drop] == 0.0) and np.all(F64(se)[drop] == 0.0)
            assert np.array_equal(C, C.T)
            h = F64(S.leverage_from_r(R, A[q], None, jp, rank, dt))
            assert abs(h.sum() - rank) <= 1e-9 * max(rank, 1)
            if rank:
                keep = jp[:rank]
                G = A[q][:, keep].T @ A[q][:, keep]
                assert np.linalg.norm(C[np.ix_(keep, keep)] @ G / 2.0 - np.eye(rank)) <= 1e-7


def test_byte_formula_takes_the_required_shapes():
    assert S.max_rows(31) == 512 and S.max_rows(63) >= 256 and S.max_rows(0) == 0 and S.max_rows(64) == 0
    for m, n in S.FIT_SHAPES:
        assert n <= m <= S.max_rows(n)
    assert S.fit_wave_route(64, 31) and not S.fit_wave_route(65, 31) and not S.fit_wave_route(64, 32)
