"""CPU checks of tests/batched_update_ref.py, the restatement the GPU test of section 8d measures the kernels against: it agrees with the
Householder references of hp_ref.py where they overlap, keeps the signed Gram matrix, reports the two failures, and is exactly
homogeneous under scaling by a power of two."""
import numpy as np

import batched_update_ref as U
import hp_ref as H

EPS = H.EPS


def _rows(seed, m, n):
    return np.random.default_rng(seed).standard_normal((m, n))


def _f(x):
    return np.asarray(x, dtype=np.float64)


def test_without_removed_rows_it_is_the_row_append_update():
    """hp_ref.append_rows is dgeqr2 of [R ; B]: the zeros below R's diagonal stay zeros, so R' and V are the same numbers up to the order
    of the sums of squares"""
    for n, p in ((1, 1), (5, 3), (17, 40), (32, 64)):
        R = np.triu(np.linalg.qr(_rows(n, 2 * n + 3, n), mode="r"))
        B = _rows(100 + n, p, n)
        Rn, V, tau, _, _, info = U.update(R, B, p, dtype=np.float64)
        F, t = H.append_rows(R, B, np.float64)
        assert info == 0
        scale = np.linalg.norm(R) + np.linalg.norm(B)
        assert np.linalg.norm(np.triu(Rn) - H.triu(F)) <= 4 * n * EPS * scale
        assert np.linalg.norm(V - F[n:]) <= 4 * n * EPS * np.linalg.norm(F[n:])
        assert np.linalg.norm(tau - t) <= 4 * n * EPS
        assert np.all(np.tril(F[:n], -1) == 0.0)


def test_a_removal_agrees_with_the_householder_qr_of_the_surviving_rows_in_extended_precision():
    for n, p_add, p_del, surv in ((4, 0, 5, 12), (8, 3, 2, 16), (15, 17, 16, 40), (32, 0, 32, 40)):
        rng = np.random.default_rng(10 * n + p_del)
        allrows = rng.standard_normal((surv - p_add + p_del, n))
        gone = np.sort(rng.choice(len(allrows), p_del, replace=False))
        keep = np.setdiff1d(np.arange(len(allrows)), gone)
        new = rng.standard_normal((p_add, n))
        R = H.triu(H.qr(allrows)[0])
        Rn, _, _, _, _, info = U.update(R, np.vstack([new, allrows[gone]]), p_add, dtype=H.LD)
        assert info == 0
        Rl = H.remove_rows(np.vstack([allrows, new]), np.concatenate([keep, len(allrows) + np.arange(p_add)]))
        sg = np.sign(_f(np.diag(Rl))) * np.sign(_f(np.diag(Rn)))
        kappa = np.linalg.cond(_f(Rl))
        err = float(H.norm(H.arr(Rn) - H.arr(sg)[:, None] * Rl) / H.norm(Rl))
        assert err <= 50 * kappa * H.EPS_LD, (n, err / H.EPS_LD, kappa)


def test_the_signed_gram_matrix_and_the_signed_column_norms_are_kept():
    n, nrhs, p_add, p_del = 12, 3, 7, 6
    rng = np.random.default_rng(12)
    kept, old, new = rng.standard_normal((30, n)), rng.standard_normal((p_del, n)), rng.standard_normal((p_add, n))
    R = np.triu(np.linalg.qr(np.vstack([kept, old]), mode="r"))
    B = np.vstack([new, old])
    C1, C2 = rng.standard_normal((n, nrhs)), rng.standard_normal((p_add + p_del, nrhs))
    Rn, V, tau, Z, E, info = U.update(R, B, p_add, C1, C2)
    assert info == 0
    G0 = R.T @ R
    assert np.linalg.norm(Rn.T @ Rn - (G0 + new.T @ new - old.T @ old)) <= n * EPS * np.linalg.norm(G0)
    S = np.where(np.arange(p_add + p_del) < p_add, 1.0, -1.0)[:, None]
    before = (C1 * C1).sum(axis=0) + (S * C2 * C2).sum(axis=0)
    after = (Z * Z).sum(axis=0) + (S * E * E).sum(axis=0)
    scale = (C1 * C1).sum(axis=0) + (C2 * C2).sum(axis=0)
    assert np.max(np.abs(after - before) / scale) <= (n + p_add + p_del) * EPS
    Z2, E2 = U.apply(V, tau, p_add, C1, C2)          # the stored reflectors reproduce the ride-along result exactly: the same operations
    assert np.array_equal(Z2, Z) and np.array_equal(E2, E)
    assert np.all(np.tril(Rn, -1) == 0.0)


def test_the_two_failures_leave_everything_as_it_was():
    n, nrhs = 6, 2
    rng = np.random.default_rng(6)
    A, Bm = rng.standard_normal((20, n)), rng.standard_normal((20, nrhs))
    R = np.triu(np.linalg.qr(A, mode="r"))
    stranger = 10.0 * rng.standard_normal((1, n))           # a row that was never added: d = R(0,0)^2 - b_0^2 < 0 in some column
    Rn, V, tau, _, _, info = U.update(R, stranger, 0)
    assert 1 <= info <= n
    assert np.array_equal(Rn, R) and np.array_equal(V, stranger) and np.all(tau == 0.0)
    acc = U.Accumulator(n, nrhs)
    assert acc.step(A[:n + 1], Bm[:n + 1], A[:0], Bm[:0]) == 0 and acc.rows == n + 1
    state = (acc.R.copy(), acc.Z.copy(), acc.rss.copy(), acc.rows)
    assert acc.step(A[:0], Bm[:0], A[:2], Bm[:2]) == -1                  # n - 1 rows would be left
    assert acc.step(A[:0], Bm[:0], stranger, Bm[:1]) >= 1
    assert np.array_equal(acc.R, state[0]) and np.array_equal(acc.Z, state[1]) and np.array_equal(acc.rss, state[2]) and acc.rows == state[3]
    assert acc.step(A[:0], Bm[:0], A[:1], Bm[:1]) == 0 and acc.rows == n  # exactly n rows left: legal
    X = H.solve_r(acc.R, acc.Z, np.float64)
    Xn = np.linalg.lstsq(A[1:n + 1], Bm[1:n + 1], rcond=None)[0]
    assert np.linalg.norm(X - Xn) <= 1e3 * np.linalg.cond(A[1:n + 1]) ** 2 * EPS * np.linalg.norm(Xn)


def test_exact_homogeneity_under_a_power_of_two():
    n, nrhs, p_add, p_del = 9, 2, 5, 4
    rng = np.random.default_rng(9)
    kept, old, new = rng.standard_normal((20, n)), rng.standard_normal((p_del, n)), rng.standard_normal((p_add, n))
    R = np.triu(np.linalg.qr(np.vstack([kept, old]), mode="r"))
    B = np.vstack([new, old])
    C1, C2 = rng.standard_normal((n, nrhs)), rng.standard_normal((p_add + p_del, nrhs))
    s, r = 2.0 ** 40, 2.0 ** -77
    for dtype in (np.float64, H.LD):
        a = U.update(R, B, p_add, C1, C2, dtype)
        b = U.update(s * R, s * B, p_add, r * C1, r * C2, dtype)
        assert a[5] == 0 and b[5] == 0
        assert np.all(b[0] == H.arr(s, dtype) * a[0]) and np.all(b[1] == a[1]) and np.all(b[2] == a[2])
        assert np.all(b[3] == H.arr(r, dtype) * a[3]) and np.all(b[4] == H.arr(r, dtype) * a[4])
    bad = B.copy()
    bad[p_add:] *= 10.0
    assert U.update(R, bad, p_add)[5] == U.update(s * R, s * bad, p_add)[5] != 0
