"""-m gpu: batched column-pivoted QR and rank-deficient least squares (mi355x_qr.h section 8b), matrix by matrix.

The yardstick for the factors is `_dlaqp2` below, a numpy restatement of LAPACK's unblocked dgeqp3 (dlarfg signs, the partial norms
downdated by vn1 *= sqrt(max(0, 1 - (|A(j,c)| / vn1)^2)) and recomputed when that times (vn1 / vn2)^2 is at most sqrt(eps), the first
maximum on a tie); for solutions, residuals and ranks it is numpy.linalg.lstsq / svd.  The shapes are those of test_gpu_batched.py with
smaller batches: both routes, every register width of the wave route, a square matrix, the LDS edge, a batch that is no multiple of
four, more workgroups than the chip has CUs.

Bounds: (n + 8) eps for ||A P - Q R|| / ||A|| and ||Q^T Q - I|| (test_gpu_batched.py); TOL = 100 sqrt(eps) for the pivoting properties
(test_gpu_pivot.py: LAPACK keeps a downdated norm while its estimated relative error is below sqrt(eps)); 50 kappa eps for R, V and
tau against the restatement where the pivot order agrees; 50 (kappa_r + kappa_r^2 |r| / (|A| |X|)) eps for solutions against numpy with
kappa_r = sigma_1 / sigma_r; 100 |A| |x_j| eps |r_j| for |resid^2 - |r_j|^2|.  On the CPU the restatement (with the solve written
out the same way) gave the true rank on all nine rank shapes in 20 draws each, and sat at 0.006 to 0.09 of the solution bound.

Right-hand sides.  The residual bound is proportional to |A| |x_j|, while the rounding error of any ||(Q^T b)(r..m)|| is proportional
to |b|: the bound means something only for a b whose fitted part is not negligible beside |b|.  A Gaussian b against a rank-1 matrix
of 64 rows has a fitted part of |b| / 8 on average and of |b| / 100 in one column out of ten, where no algorithm meets the bound.  So
`_rhs` builds b = f + e with f in range(A), e orthogonal to it, and |f| = |e|: then |A| |x_j| >= |f| = |b| / sqrt(2) for every column.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TOL = 100 * np.sqrt(EPS)
SENTINEL = -7.25e33


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


def _rand(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape)


def _up(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _down(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _pack(A):
    """(batch, rows, cols) -> the packed column-major batch as a (batch, cols, rows) array"""
    return np.ascontiguousarray(A.transpose(0, 2, 1))


def _nrm(X):
    return np.sqrt((X * X).reshape(X.shape[0], -1).sum(axis=1))


def _unit_lower(F):
    n = F.shape[1]
    V = np.tril(F, -1)
    V[np.arange(n), np.arange(n)] = 1.0
    return V


def _dlaqp2(A):
    """LAPACK dlaqp2 with every column free: (F, tau, jpvt), F in dgeqr2's layout, jpvt 0-based"""
    F = np.array(A, dtype=np.float64)
    m, n = F.shape
    jpvt, tau = np.arange(n), np.zeros(n)
    vn1 = np.sqrt((F * F).sum(axis=0))
    vn2 = vn1.copy()
    for j in range(n):
        p = j + int(np.argmax(vn1[j:]))                    # (argmax returns the first maximum: the lowest index on a tie)
        if p != j:
            F[:, [j, p]] = F[:, [p, j]]
            jpvt[[j, p]] = jpvt[[p, j]]
            vn1[p], vn2[p] = vn1[j], vn2[j]
        x = F[j + 1:, j]
        ssq = float(x @ x)
        if ssq != 0.0:
            alpha = F[j, j]
            beta = -np.copysign(np.hypot(alpha, np.sqrt(ssq)), alpha)
            tau[j] = (beta - alpha) / beta
            v = np.concatenate(([1.0], x / (alpha - beta)))
            F[j:, j + 1:] -= tau[j] * np.outer(v, v @ F[j:, j + 1:])
            F[j, j] = beta
            F[j + 1:, j] = v[1:]
        for c in range(j + 1, n):
            if vn1[c] == 0.0:
                continue
            t = abs(F[j, c]) / vn1[c]
            temp = max(0.0, 1.0 - t * t)
            if temp * (vn1[c] / vn2[c]) ** 2 <= np.sqrt(EPS):
                vn1[c] = vn2[c] = np.sqrt(float(F[j + 1:, c] @ F[j + 1:, c]))
            else:
                vn1[c] *= np.sqrt(temp)
    return F, tau, jpvt


def _ints(*shape, fill=-9):
    return _up(np.full(shape, fill, dtype=np.int32))


def _geqp3(plan, A, with_q=True):
    """packed call: F (batch, m, n), tau (batch, n), jpvt (batch, n), Q (batch, m, n)"""
    batch, m, n = A.shape
    dA, dtau, dj = _up(_pack(A)), _up(np.full((batch, n), SENTINEL)), _ints(batch, n)
    plan.geqp3_batched(dA, m, n, m, m * n, dj, n, dtau, n, batch)
    dQ = None
    if with_q:
        dQ = _up(np.full((batch, n, m), SENTINEL))
        plan.orgqr_batched(dA, m, n, m, m * n, dtau, n, dQ, m, m * n, batch)
    plan.sync()
    return (_down(dA).transpose(0, 2, 1), _down(dtau), _down(dj).astype(np.int64),
            _down(dQ).transpose(0, 2, 1) if with_q else None)


def _solve(plan, A, Bm, minnorm, rcond=None):
    """packed gelsy (minnorm) or gelsp: X (batch, n, nrhs), resid (batch, nrhs), rank (batch,), jpvt, then everything the call left:
    F, tau, the tail of Q^T B (batch, m - n, nrhs)"""
    batch, m, n = A.shape
    nrhs = Bm.shape[2]
    dA, dtau, dj, dB = _up(_pack(A)), _up(np.full((batch, n), SENTINEL)), _ints(batch, n), _up(_pack(Bm))
    dres, drank = _up(np.full((batch, nrhs), SENTINEL)), _ints(batch)
    call = plan.gelsy_batched if minnorm else plan.gelsp_batched
    call(dA, m, n, m, m * n, dj, n, dtau, n, dB, nrhs, m, m * nrhs, batch, rcond=rcond, dresid=dres, drank=drank)
    plan.sync()
    Y = _down(dB).transpose(0, 2, 1)
    return (Y[:, :n, :].copy(), _down(dres), _down(drank).astype(np.int64), _down(dj).astype(np.int64), _down(dA).transpose(0, 2, 1),
            _down(dtau), Y[:, n:, :].copy())


def _check_pivoting(R):
    """the diagonal decreases and dominates every trailing partial column norm, to TOL, above the rounding floor (test_gpu_pivot.py)"""
    n = R.shape[0]
    d = np.abs(np.diag(R))
    live = d > n * EPS * d[0]
    S = np.cumsum((R * R)[::-1], axis=0)[::-1]           # S[j, k] = sum_{i >= j} R[i, k]^2
    for j in range(n - 1):
        if not live[j]:
            continue
        assert d[j + 1] <= d[j] * (1 + TOL), (j, d[j], d[j + 1])
        best = np.sqrt(S[j, j + 1:].max())
        assert d[j] >= (1 - TOL) * best, (j, d[j], best)


def _check_factors(A, F, tau, jp, Q):
    """check 1 of the section's tests on a whole batch; returns the worst residual and orthogonality in eps"""
    batch, m, n = A.shape
    assert np.all(np.sort(jp, axis=1) == np.arange(n)), "jpvt is not a permutation"
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(tau)) and np.all(np.isfinite(Q))
    R = np.triu(F[:, :n, :])
    AP = np.take_along_axis(A, jp[:, None, :], axis=2)
    an = _nrm(A)
    resid = _nrm(AP - Q @ R) / np.where(an > 0, an, 1.0)
    orth = _nrm(Q.transpose(0, 2, 1) @ Q - np.eye(n))
    assert resid.max() <= (n + 8) * EPS, resid.max() / EPS
    assert orth.max() <= (n + 8) * EPS, orth.max() / EPS
    if m == n:
        assert np.all(tau[:, n - 1] == 0.0)
    for q in range(batch):
        _check_pivoting(R[q])
    return resid.max() / EPS, orth.max() / EPS


def _check_against_mirror(A, F, tau, jp, kappa):
    """check 2: the same pivot order as the restatement, or a difference only where the two candidates' partial norms agree to TOL;
    where the order agrees, R, V and tau within 50 kappa eps.  Returns (matrices whose order differed, the worst multiple of kappa eps)"""
    m, n = A.shape
    Fm, taum, jpm = _dlaqp2(A)
    if not np.array_equal(jp, jpm):
        j = int(np.argmax(jp != jpm))
        Qj = np.linalg.qr(A[:, jpm[:j]])[0] if j else np.zeros((m, 0))
        res = A[:, [jp[j], jpm[j]]]
        res = res - Qj @ (Qj.T @ res)
        na, nb = np.linalg.norm(res, axis=0)
        assert abs(na - nb) <= TOL * max(na, nb), (j, na, nb)
        return 1, 0.0
    R, Rm = np.triu(F[:n]), np.triu(Fm[:n])
    V, Vm = _unit_lower(F), _unit_lower(Fm)
    worst = max(np.linalg.norm(R - Rm) / np.linalg.norm(Rm), np.linalg.norm(V - Vm) / np.linalg.norm(Vm),
                np.linalg.norm(tau - taum)) / (kappa * EPS)
    assert worst <= 50, worst
    return 0, worst


WAVE = [(1, 1, 1), (5, 3, 3), (17, 17, 5), (33, 8, 7), (64, 32, 9), (8, 4, 4099)]
WG = [(65, 4, 3), (64, 64, 2), (100, 33, 5), (300, 40, 3), (256, 64, 2), (512, 32, 2)]


@pytest.mark.parametrize("m,n,batch", WAVE + WG)
def test_factors_and_pivoting_on_gaussian_input(qr, plan, m, n, batch):
    A = _rand(1000 * m + n, batch, m, n)
    F, tau, jp, Q = _geqp3(plan, A)
    er, eo = _check_factors(A, F, tau, jp, Q)
    differ, worst = 0, 0.0
    for q in list(range(min(batch, 8))) + ([batch - 1] if batch > 8 else []):     # (the restatement is slow: the ends of a long batch)
        d, w = _check_against_mirror(A[q], F[q], tau[q], jp[q], np.linalg.cond(A[q]))
        differ, worst = differ + d, max(worst, w)
    print(f"batched geqp3 {m}x{n} x{batch}: resid {er:.2f} eps, orth {eo:.2f} eps (bound {n + 8}); against the restatement: order differs "
          f"in {differ}, factors within {worst:.2f} kappa eps (bound 50)")


def _graded(m, n, ratio, rng):
    U = np.linalg.qr(rng.standard_normal((m, n)))[0]
    s = ratio ** np.arange(n)
    pi = rng.permutation(n)
    A = np.empty((m, n))
    A[:, pi] = U * s
    return A, s, pi


@pytest.mark.parametrize("m,n", [(64, 32), (100, 33)])
def test_exact_pivot_order_on_graded_orthogonal_columns(qr, plan, m, n):
    rng = np.random.default_rng(m + n)
    As, pis = zip(*[_graded(m, n, 0.9, rng)[::2] for _ in range(3)])
    A, kappa = np.stack(As), 0.9 ** -(n - 1)
    F, tau, jp, Q = _geqp3(plan, A)
    _check_factors(A, F, tau, jp, Q)
    for q in range(3):
        assert np.array_equal(jp[q], pis[q])                                  # the descending-norm order
        Fm, taum, jpm = _dlaqp2(A[q])
        assert np.array_equal(jp[q], jpm)
        differ, worst = _check_against_mirror(A[q], F[q], tau[q], jp[q], kappa)
        assert differ == 0
        assert np.max(np.abs(np.abs(np.diag(F[q])) - 0.9 ** np.arange(n))) < 1e-12


def _rhs(A, r, nrhs, rng):
    """b = f + e: f in range(A) (rank r), e orthogonal to it, |f| = |e| (the module docstring says why); m == r: b = f"""
    m = A.shape[0]
    U = np.linalg.svd(A)[0][:, :r]
    G = rng.standard_normal((m, nrhs))
    E = G - U @ (U.T @ G)
    if r == m:
        E[...] = 0.0
    if r == 0:
        return E
    Fit = U @ rng.standard_normal((r, nrhs))
    en = np.linalg.norm(E, axis=0)
    return Fit / np.linalg.norm(Fit, axis=0) * np.where(en > 0, en, 1.0) + E


def _rank_batch(m, n, r, nrhs, seed=0):
    """five matrices: rank r at 0, 2 and 4, a full-rank one at 1, a zero one at 3; the right-hand sides of _rhs"""
    rng = np.random.default_rng(10000 * m + 100 * n + r + seed)
    ranks = [r, n, r, 0, r]
    A = np.stack([rng.standard_normal((m, k)) @ rng.standard_normal((k, n)) if 0 < k < n else
                  (rng.standard_normal((m, n)) if k == n else np.zeros((m, n))) for k in ranks])
    Bm = np.stack([_rhs(A[q], ranks[q], nrhs, rng) for q in range(5)]) if nrhs else None
    return A, Bm, np.array(ranks)


RANKS = [(5, 3, 2), (64, 29, 11), (64, 32, 1), (17, 17, 5), (100, 33, 20), (256, 64, 40), (300, 40, 39), (64, 64, 63), (512, 32, 31)]


@pytest.mark.parametrize("m,n,r", RANKS)
def test_rank_from_every_entry_point(qr, plan, m, n, r):
    A, Bm, ranks = _rank_batch(m, n, r, 2)
    batch = 5
    dA, dtau, dj, drank = _up(_pack(A)), _up(np.zeros((batch, n))), _ints(batch, n), _ints(batch + 2)
    plan.geqp3_batched(dA, m, n, m, m * n, dj, n, dtau, n, batch)
    plan.rank_batched(dA, m, n, m, m * n, drank, batch)
    plan.sync()
    got = _down(drank)
    d = np.abs(np.diagonal(_down(dA).transpose(0, 2, 1)[:, :n, :], axis1=1, axis2=2))
    print(f"rank {m}x{n} r={r}: d[r-1]/d[0] = {d[0, r - 1] / d[0, 0]:.2e}" + (f", d[r]/d[0] = {d[0, r] / d[0, 0]:.2e}" if r < n else ""))
    assert list(got) == list(ranks) + [-9, -9]
    assert [np.linalg.matrix_rank(A[q]) for q in range(batch)] == list(ranks)
    for minnorm in (False, True):
        assert list(_solve(plan, A, Bm, minnorm)[2]) == list(ranks)
    assert list(qr.lstsq_pivoted_batched(A, Bm, rcond=None)[2]) == list(ranks)
    dr2 = _ints(batch)
    plan.rank_batched(dA, m, n, m, m * n, dr2, batch, rcond=0.0)              # rcond = 0: every non-zero diagonal counts
    plan.sync()
    assert list(_down(dr2)) == [int(np.argmax(np.append(d[q], 0.0) == 0.0)) for q in range(batch)]


def _check_solutions(A, Bm, ranks, X, resid, what):
    """checks 5 of the section's tests: every matrix against numpy.linalg.lstsq at its rank; returns the worst multiples of the bounds"""
    wx = wr = 0.0
    for q in range(A.shape[0]):
        r = ranks[q]
        if r == 0:
            assert np.all(X[q] == 0.0)
            bn = np.linalg.norm(Bm[q], axis=0)
            assert np.all(np.abs(resid[q] - bn) <= 16 * EPS * bn)            # (a sum of m squares either way: (log2 m + 3) eps at most)
            continue
        Xn = np.linalg.lstsq(A[q], Bm[q], rcond=None)[0]
        rn = Bm[q] - A[q] @ Xn
        s = np.linalg.svd(A[q], compute_uv=False)
        kappa, a2 = s[0] / s[r - 1], s[0]
        bound = 50 * (kappa + kappa ** 2 * np.linalg.norm(rn) / (a2 * np.linalg.norm(Xn))) * EPS
        if what == "minnorm":
            ex = np.linalg.norm(X[q] - Xn) / np.linalg.norm(Xn)
            wx = max(wx, ex / bound)
            assert ex <= bound, (q, ex, bound)
        for j in range(Bm.shape[2]):
            rj = np.linalg.norm(rn[:, j])
            rb = 100 * a2 * np.linalg.norm(Xn[:, j]) * EPS * rj
            got = resid[q, j] ** 2 if what != "basic" else float(np.sum((A[q] @ X[q][:, j] - Bm[q][:, j]) ** 2))
            er = abs(got - rj * rj)
            if rb > 0:
                wr = max(wr, er / rb)
            assert er <= rb, (q, j, er, rb)
    return wx, wr


SOLVES = [(5, 3, 2, 1, True), (64, 29, 11, 3, True), (64, 32, 1, 2, True), (64, 32, 1, 40, False), (17, 17, 5, 4, True),
          (100, 33, 20, 2, True), (256, 64, 40, 4, False), (300, 40, 39, 1, False), (64, 64, 63, 3, False), (512, 32, 31, 1, False)]


@pytest.mark.parametrize("m,n,r,nrhs,fused", SOLVES)
def test_gelsy_matches_numpy(qr, plan, m, n, r, nrhs, fused):
    assert fused == (n + nrhs <= 64 and m <= qr.batched_max_rows(n + nrhs))      # the case sits on the route it is meant for
    A, Bm, ranks = _rank_batch(m, n, r, nrhs)
    X, resid, rank, jp, F, tau, tail = _solve(plan, A, Bm, True)
    assert list(rank) == list(ranks)
    wx, wr = _check_solutions(A, Bm, ranks, X, resid, "minnorm")
    print(f"batched gelsy {m}x{n} rank {r}, {nrhs} rhs ({'fused' if fused else 'composed'}): X at {wx:.3f} of its bound, resid^2 at "
          f"{wr:.3f} of its bound")
    # what the call leaves besides X: the factors of geqp3_batched on the same input, and the tail of Q^T B
    F0, tau0, jp0, _ = _geqp3(plan, A, with_q=False)
    if not fused:                             # (the fused kernel holds n + nrhs columns and may run on the other route: rounding apart,
        #                                        and with it the order of the columns that are rounding noise past the rank)
        assert np.array_equal(jp, jp0) and np.array_equal(F, F0) and np.array_equal(tau, tau0)
        dC = _up(_pack(Bm))
        plan.ormqr_batched("T", _up(_pack(F0)), m, n, m, m * n, _up(tau0), n, dC, nrhs, m, m * nrhs, 5)
        plan.sync()
        assert np.array_equal(tail, _down(dC).transpose(0, 2, 1)[:, n:, :])


@pytest.mark.parametrize("m,n,r,nrhs,fused", SOLVES)
def test_gelsp_basic_solution(qr, plan, m, n, r, nrhs, fused):
    A, Bm, ranks = _rank_batch(m, n, r, nrhs)
    X, resid, rank, jp, *_ = _solve(plan, A, Bm, False)
    Xy, residy, *_ = _solve(plan, A, Bm, True)
    assert list(rank) == list(ranks)
    assert np.array_equal(resid, residy)                                      # the same residual, bit for bit
    for q in range(5):
        zero_rows = np.flatnonzero(np.all(X[q] == 0.0, axis=1))
        assert zero_rows.size == n - ranks[q] and np.array_equal(zero_rows, np.sort(jp[q, ranks[q]:]))
    _, wr = _check_solutions(A, Bm, ranks, X, resid, "basic")
    _, wd = _check_solutions(A, Bm, ranks, X, resid, "dresid")
    # a consistent system: B = A X0
    X0 = _rand(m + r, 5, n, nrhs)
    Bc = A @ X0
    Xc, residc, rankc, *_ = _solve(plan, A, Bc, False)
    assert list(rankc) == list(ranks)
    a2 = np.array([np.linalg.norm(A[q], 2) for q in range(5)])
    lim = 100 * n * EPS * a2[:, None] * np.sqrt((Xc * Xc).sum(axis=1))
    rc = np.sqrt(((A @ Xc - Bc) ** 2).sum(axis=1))
    print(f"batched gelsp {m}x{n} rank {r}, {nrhs} rhs: |A X - B|^2 at {wr:.3f} of its bound, dresid^2 at {wd:.3f}; consistent: "
          f"residual at {np.max(rc[lim > 0] / lim[lim > 0]) if np.any(lim > 0) else 0.0:.3f} of its bound")
    assert np.all(rc <= lim) and np.all(residc <= lim)


@pytest.mark.parametrize("m,n,nrhs,fused", [(64, 29, 3, True), (256, 64, 4, False)])
def test_full_rank_gelsp_and_gelsy_agree_bitwise(qr, plan, m, n, nrhs, fused):
    assert fused == (n + nrhs <= 64 and m <= qr.batched_max_rows(n + nrhs))
    batch = 3
    A, Bm = _rand(3 * m + n, batch, m, n), _rand(5 * m + nrhs, batch, m, nrhs)
    Xp, rp, kp, jpp, *_ = _solve(plan, A, Bm, False)
    Xy, ry, ky, jpy, *_ = _solve(plan, A, Bm, True)
    assert np.array_equal(Xp, Xy) and np.array_equal(rp, ry) and np.array_equal(jpp, jpy)
    assert list(kp) == [n] * batch == list(ky)
    wx, wr = _check_solutions(A, Bm, [n] * batch, Xy, ry, "minnorm")
    print(f"batched gelsy {m}x{n} full rank, {nrhs} rhs: X at {wx:.3f} of its bound, resid^2 at {wr:.3f}")


@pytest.mark.parametrize("m,n", [(33, 8), (100, 33)])
def test_ties_and_zeros(qr, plan, m, n):
    rng = np.random.default_rng(m * n)
    A = rng.standard_normal((4, m, n))
    A[0, :, 5] = A[0, :, 2] = 3.0 * A[0, :, 2]           # two identical columns, the largest of the matrix: the tie is at step 0
    A[1] = 0.0
    A[2, :, 4] = 0.0
    Bm = rng.standard_normal((4, m, 2))
    F, tau, jp, Q = _geqp3(plan, A)
    _check_factors(A, F, tau, jp, Q)
    assert jp[0, 0] == 2 and jp[0, 1] != 5               # the lower index first; its twin has nothing left and is not next
    assert np.array_equal(jp[1], np.arange(n)) and np.all(tau[1] == 0.0) and np.all(F[1] == 0.0)
    assert jp[2, n - 1] == 4
    X, resid, rank, jps, *_ = _solve(plan, A, Bm, True)
    assert list(rank) == [n - 1, 0, n - 1, n]
    assert np.array_equal(jps, jp)
    assert np.all(X[1] == 0.0)
    bn = np.linalg.norm(Bm[1], axis=0)
    assert np.all(np.abs(resid[1] - bn) <= 16 * EPS * bn)
    assert np.all(X[2, 4] == 0.0)                          # minimum norm: nothing on a zero column


@pytest.mark.parametrize("m,n", [(33, 8), (100, 33)])
def test_padded_layout_is_respected_and_equals_the_packed_call(qr, plan, m, n):
    batch, nrhs, tail = 5, 3, 13
    A, Bm, ranks = _rank_batch(m, n, n // 2, nrhs, seed=1)
    lda, ldb = m + 3, m + 1
    sa, st, sj, sb = lda * n + 5, n + 2, n + 3, ldb * nrhs + 4
    view = lambda b, s, ld, cols, rows: np.lib.stride_tricks.as_strided(b, (batch, cols, rows), (b.itemsize * s, b.itemsize * ld, b.itemsize))
    for minnorm in (None, False, True):                                        # geqp3, gelsp, gelsy
        abuf, tbuf, bbuf = np.full(batch * sa + tail, SENTINEL), np.full(batch * st + tail, SENTINEL), np.full(batch * sb + tail, SENTINEL)
        jbuf = np.full(batch * sj + tail, -9, dtype=np.int32)
        view(abuf, sa, lda, n, m)[...] = A.transpose(0, 2, 1)
        view(bbuf, sb, ldb, nrhs, m)[...] = Bm.transpose(0, 2, 1)
        dA, dtau, dj, dB = _up(abuf), _up(tbuf), _up(jbuf), _up(bbuf)
        if minnorm is None:
            plan.geqp3_batched(dA, m, n, lda, sa, dj, sj, dtau, st, batch)
            F, tau, jp, _ = _geqp3(plan, A, with_q=False)
        else:
            dres, drank = _up(np.full(batch * nrhs + 3, SENTINEL)), _ints(batch + 3)
            (plan.gelsy_batched if minnorm else plan.gelsp_batched)(dA, m, n, lda, sa, dj, sj, dtau, st, dB, nrhs, ldb, sb, batch,
                                                                    dresid=dres, drank=drank)
            X, resid, rank, jp, F, tau, tl = _solve(plan, A, Bm, minnorm)
        plan.sync()
        a2, t2, j2, b2 = _down(dA).copy(), _down(dtau).copy(), _down(dj).copy(), _down(dB).copy()
        assert np.array_equal(view(a2, sa, lda, n, m).transpose(0, 2, 1), F)
        assert np.array_equal(view(t2, st, n, 1, n)[:, 0, :], tau)
        assert np.array_equal(view(j2, sj, n, 1, n)[:, 0, :], jp)
        view(a2, sa, lda, n, m)[...] = SENTINEL
        view(t2, st, n, 1, n)[...] = SENTINEL
        view(j2, sj, n, 1, n)[...] = -9
        assert np.all(a2 == SENTINEL) and np.all(t2 == SENTINEL) and np.all(j2 == -9)      # gaps and tails came back intact
        if minnorm is not None:
            Y = view(b2, sb, ldb, nrhs, m).transpose(0, 2, 1)
            assert np.array_equal(Y[:, :n, :], X) and np.array_equal(Y[:, n:, :], tl)
            r2, k2 = _down(dres), _down(drank)
            assert np.array_equal(r2[:batch * nrhs].reshape(batch, nrhs), resid) and np.all(r2[batch * nrhs:] == SENTINEL)
            assert list(k2) == list(rank) + [-9] * 3
            view(b2, sb, ldb, nrhs, m)[...] = SENTINEL
            assert np.all(b2 == SENTINEL)


@pytest.mark.parametrize("m,n", [(64, 32), (100, 33)])
def test_result_is_independent_of_position_and_batch_and_repeats_bitwise(qr, plan, m, n):
    A = _rand(31 * m + n, 9, m, n)
    A[0] *= 0.8 ** np.arange(n)                            # graded columns: rcond = 0.5 below cuts the rank to a few
    A[2] = _rand(5, m, n // 3) @ _rand(6, n // 3, n)       # a rank-deficient neighbour
    A[4] = A[0]
    A[8] = A[0]

    def same(x, y):
        return all(np.array_equal(u, v) for u, v in zip(x, y))

    def at(x, q):
        return [u[q] for u in x]

    f = _geqp3(plan, A)
    assert same(at(f, 4), at(f, 0)) and same(at(f, 8), at(f, 0))
    assert same(at(_geqp3(plan, A[:1]), 0), at(f, 0))
    assert same(_geqp3(plan, A), f)
    for nrhs in (2, 40):                                   # fused and composed
        Bm = _rand(nrhs, 9, m, nrhs)
        Bm[4] = Bm[0]
        Bm[8] = Bm[0]
        for minnorm in (False, True):
            s = _solve(plan, A, Bm, minnorm, rcond=0.5)    # (the sweep of gelsy runs on every matrix)
            assert 0 < s[2][0] < n
            assert same(at(s, 4), at(s, 0)) and same(at(s, 8), at(s, 0))
            assert same(at(_solve(plan, A[:1], Bm[:1], minnorm, rcond=0.5), 0), at(s, 0))
            assert same(_solve(plan, A, Bm, minnorm, rcond=0.5), s)


def test_unpivoted_factorisation_is_unchanged_by_a_pivoted_call_on_the_plan(qr, plan):
    m, n, batch = 100, 33, 3
    A = _rand(77, batch, m, n)
    outs = []
    for k in range(2):
        dA, dtau = _up(_pack(A)), _up(np.zeros((batch, n)))
        plan.geqrf_batched(dA, m, n, m, m * n, dtau, n, batch)
        plan.sync()
        outs.append((_down(dA).copy(), _down(dtau).copy()))
        if k == 0:
            _solve(plan, A, _rand(78, batch, m, 2), True)
            _geqp3(plan, A)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# (5, 3), (16, 4): geqp3 takes the 4-register wave kernel, geqrf the 8-register one; (64, 28): 32 registers; (65, 8): the first row count
# of the workgroup route
PERMUTED = [(5, 3), (16, 4), (64, 28), (65, 8), (100, 33), (256, 64)]


@pytest.mark.parametrize("m,n", PERMUTED)
def test_factors_equal_geqrf_on_permuted_columns_bitwise(qr, plan, m, n):
    """The pivoted kernels run the unpivoted kernels' column step: geqrf on A[:, jpvt] returns geqp3's factors and tau bit for bit."""
    batch = 5                                              # (a partly filled workgroup on the wave route)
    rng = np.random.default_rng(7000 * m + n)
    A = rng.standard_normal((batch, m, n)) * 2.0 ** rng.uniform(-3.0, 3.0, (batch, 1, n))
    for q in range(batch):                                 # the largest column is not the first: step 0 swaps in every member
        if np.argmax(np.linalg.norm(A[q], axis=0)) == 0:
            A[q][:, [0, 1]] = A[q][:, [1, 0]]
    F, tau, jp, _ = _geqp3(plan, A, with_q=False)
    assert np.all(np.sort(jp, axis=1) == np.arange(n))
    assert not np.any(np.all(jp == np.arange(n), axis=1)), "a member was not permuted: the comparison would be vacuous"
    AP = np.take_along_axis(A, jp[:, None, :], axis=2)
    dA, dtau = _up(_pack(AP)), _up(np.full((batch, n), SENTINEL))
    plan.geqrf_batched(dA, m, n, m, m * n, dtau, n, batch)
    plan.sync()
    F0, tau0 = _down(dA).transpose(0, 2, 1), _down(dtau)
    print(f"geqp3 against geqrf on the permuted columns {m}x{n}: {int(np.sum(F != F0))} factor entries and {int(np.sum(tau != tau0))} tau differ")
    assert np.array_equal(F, F0) and np.array_equal(tau, tau0)


def test_host_twins_and_python_wrappers(qr):
    m, n, nrhs = 20, 6, 3
    A, Bm, ranks = _rank_batch(m, n, 4, nrhs)
    Q, R, jp = qr.qr_pivoted_batched(A)
    assert Q.shape == (5, m, n) and R.shape == (5, n, n) and jp.shape == (5, n)
    AP = np.take_along_axis(A, jp[:, None, :], axis=2)
    assert (_nrm(AP - Q @ R) / np.maximum(_nrm(A), 1e-300)).max() <= (n + 8) * EPS
    assert _nrm(Q.transpose(0, 2, 1) @ Q - np.eye(n)).max() <= (n + 8) * EPS
    assert np.all(np.tril(R, -1) == 0.0)
    X, resid, rank, jp2 = qr.lstsq_pivoted_batched(A, Bm)
    assert X.shape == (5, n, nrhs) and resid.shape == (5, nrhs) and np.array_equal(jp2, jp)
    assert list(rank) == list(ranks)
    _check_solutions(A, Bm, ranks, X, resid, "minnorm")
    Xp, residp, rankp, _ = qr.lstsq_pivoted_batched(A, Bm, minnorm=False)
    assert list(rankp) == list(ranks) and np.array_equal(residp, resid)
    for q in range(5):
        assert np.array_equal(np.flatnonzero(np.all(Xp[q] == 0.0, axis=1)), np.sort(jp[q, ranks[q]:]))
    # the C entry point itself on a zero matrix: status 0, rank 0, resid and rank and jpvt optional
    Z, Bz, Xz = np.zeros((1, n, m)), _pack(_rand(3, 1, m, nrhs)), np.full((1, nrhs, n), SENTINEL)
    dp = C.POINTER(C.c_double)
    rc = qr.lib.qr_lstsq_pivoted_batched(Z.ctypes.data_as(dp), m, n, Bz.ctypes.data_as(dp), nrhs, 1, -1.0, 1, Xz.ctypes.data_as(dp), None,
                                         None, None)
    assert rc == 0 and np.all(Xz == 0.0)
