"""-m gpu: the batched interface (mi355x_qr.h section 8) against numpy / LAPACK, matrix by matrix.

Seeded standard_normal inputs.  The shapes are the smallest at which a route, an edge or an index can go wrong: the wave route (m <= 64,
<= 32 columns held) at each register width, a batch that is no multiple of the four matrices of a workgroup, more than 4096 matrices;
the workgroup route just past each limit of the wave route and at both ends of qr_batched_max_rows.

Bounds: (n + 8) eps for the residual and the orthogonality (a numpy restatement of the unblocked algorithm stayed below 0.45 (n + 8) eps
and 2.5 eps on these shapes), 50 kappa eps for R, V and tau against LAPACK's (the project's bound for R against LAPACK; the restatement
stayed within 6.3 kappa eps), 50 (kappa + kappa^2 |r| / (|A| |X|)) eps for least-squares solutions (the bound of test_gpu_lstsq.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
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


def _factor(plan, A, with_q=True):
    """packed call: returns F (batch, m, n), tau (batch, n), Q (batch, m, n)"""
    batch, m, n = A.shape
    dA, dtau = _up(_pack(A)), _up(np.full((batch, n), SENTINEL))
    plan.geqrf_batched(dA, m, n, m, m * n, dtau, n, batch)
    dQ = None
    if with_q:
        dQ = _up(np.full((batch, n, m), SENTINEL))
        plan.orgqr_batched(dA, m, n, m, m * n, dtau, n, dQ, m, m * n, batch)
    plan.sync()
    return _down(dA).transpose(0, 2, 1), _down(dtau), (_down(dQ).transpose(0, 2, 1) if with_q else None)


def _lapack(A):
    """numpy.linalg.qr(mode='raw') per matrix: F (batch, m, n), tau (batch, n)"""
    F, tau = np.empty_like(A), np.empty((A.shape[0], A.shape[2]))
    for q in range(A.shape[0]):
        h, t = np.linalg.qr(A[q], mode="raw")
        F[q], tau[q] = h.T, t
    return F, tau


def _nrm(X):
    return np.sqrt((X * X).reshape(X.shape[0], -1).sum(axis=1))


def _unit_lower(F):
    n = F.shape[2]
    V = np.tril(F, -1)
    V[:, np.arange(n), np.arange(n)] = 1.0
    return V


WAVE = [(1, 1, 1), (5, 3, 3), (17, 17, 5), (33, 8, 7), (64, 1, 4), (64, 32, 130), (8, 4, 4099)]
WG = [(65, 4, 3), (64, 64, 2), (100, 33, 37), (300, 40, 3), (256, 64, 2), (512, 32, 2)]


@pytest.mark.parametrize("m,n,batch", WAVE + WG)
def test_factorisation_against_lapack(qr, plan, m, n, batch):
    A = _rand(1000 * m + n, batch, m, n)
    F, tau, Q = _factor(plan, A)
    R = np.triu(F[:, :n, :])
    I = np.eye(n)
    resid = _nrm(A - Q @ R) / _nrm(A)
    orth = _nrm(Q.transpose(0, 2, 1) @ Q - I)
    Fl, taul = _lapack(A)
    kappa = np.linalg.cond(A)
    Rl = np.triu(Fl[:, :n, :])
    er = _nrm(R - Rl) / _nrm(Rl) / (kappa * EPS)
    et = _nrm(tau - taul) / (kappa * EPS)
    V, Vl = _unit_lower(F), _unit_lower(Fl)
    ev = _nrm(V - Vl) / _nrm(Vl) / (kappa * EPS)
    print(f"batched {m}x{n} x{batch}: resid {resid.max() / EPS:.2f} eps, orth {orth.max() / EPS:.2f} eps (bound {n + 8}); against LAPACK in "
          f"kappa eps: R {er.max():.2f}, tau {et.max():.2f}, V {ev.max():.2f} (bound 50)")
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(tau)) and np.all(np.isfinite(Q))
    assert resid.max() <= (n + 8) * EPS
    assert orth.max() <= (n + 8) * EPS
    assert er.max() <= 50 and et.max() <= 50 and ev.max() <= 50
    if m == n:
        assert np.all(tau[:, n - 1] == 0.0)            # the last column of a square matrix has nothing below it


@pytest.mark.parametrize("m,n,batch", [(33, 8, 7), (100, 33, 5)])
def test_padded_layout_is_respected_and_equals_the_packed_call(qr, plan, m, n, batch):
    A = _rand(7 * m + n, batch, m, n)
    F, tau, Q = _factor(plan, A)
    lda, ldq = m + 3, m + 2
    sa, st, sq, tail = lda * n + 5, n + 2, ldq * n + 11, 13
    abuf = np.full(batch * sa + tail, SENTINEL)
    tbuf = np.full(batch * st + tail, SENTINEL)
    qbuf = np.full(batch * sq + tail, SENTINEL)
    view = lambda b, s, ld, cols, rows: np.lib.stride_tricks.as_strided(b, (batch, cols, rows), (8 * s, 8 * ld, 8))
    view(abuf, sa, lda, n, m)[...] = A.transpose(0, 2, 1)
    dA, dtau, dQ = _up(abuf), _up(tbuf), _up(qbuf)
    plan.geqrf_batched(dA, m, n, lda, sa, dtau, st, batch)
    plan.orgqr_batched(dA, m, n, lda, sa, dtau, st, dQ, ldq, sq, batch)
    plan.sync()
    a2, t2, q2 = _down(dA).copy(), _down(dtau).copy(), _down(dQ).copy()
    assert np.array_equal(view(a2, sa, lda, n, m).transpose(0, 2, 1), F)
    assert np.array_equal(view(t2, st, n, 1, n)[:, 0, :], tau)
    assert np.array_equal(view(q2, sq, ldq, n, m).transpose(0, 2, 1), Q)
    view(a2, sa, lda, n, m)[...] = SENTINEL
    view(t2, st, n, 1, n)[...] = SENTINEL
    view(q2, sq, ldq, n, m)[...] = SENTINEL
    assert np.all(a2 == SENTINEL) and np.all(t2 == SENTINEL) and np.all(q2 == SENTINEL)      # gaps and tails came back intact
    # the same for ormqr and gels: C / B with a padded layout
    nrhs = 3
    Bm = _rand(m, batch, m, nrhs)
    ldb = m + 1
    sb = ldb * nrhs + 4
    bbuf = np.full(batch * sb + tail, SENTINEL)
    view(bbuf, sb, ldb, nrhs, m)[...] = Bm.transpose(0, 2, 1)
    dC = _up(bbuf)
    plan.ormqr_batched("T", dA, m, n, lda, sa, dtau, st, dC, nrhs, ldb, sb, batch)
    plan.sync()
    c2 = _down(dC).copy()
    dCp = _up(_pack(Bm))
    dFp, dtp = _up(_pack(F)), _up(tau)
    plan.ormqr_batched("T", dFp, m, n, m, m * n, dtp, n, dCp, nrhs, m, m * nrhs, batch)
    plan.sync()
    assert np.array_equal(view(c2, sb, ldb, nrhs, m), _down(dCp))
    view(c2, sb, ldb, nrhs, m)[...] = SENTINEL
    assert np.all(c2 == SENTINEL)
    view(abuf, sa, lda, n, m)[...] = A.transpose(0, 2, 1)
    dA, dB, dinfo = _up(abuf), _up(bbuf), _up(np.full(batch + 3, -9, dtype=np.int32))
    plan.gels_batched(dA, m, n, lda, sa, dtau, st, dB, nrhs, ldb, sb, dinfo, batch)
    plan.sync()
    b2, i2 = _down(dB).copy(), _down(dinfo)
    dAp, dBp, dip = _up(_pack(A)), _up(_pack(Bm)), _up(np.full(batch, -9, dtype=np.int32))
    plan.gels_batched(dAp, m, n, m, m * n, dtp, n, dBp, nrhs, m, m * nrhs, dip, batch)
    plan.sync()
    assert np.array_equal(view(b2, sb, ldb, nrhs, m), _down(dBp))
    assert list(i2) == [0] * batch + [-9] * 3 and not _down(dip).any()
    view(b2, sb, ldb, nrhs, m)[...] = SENTINEL
    assert np.all(b2 == SENTINEL)


@pytest.mark.parametrize("m,n", [(64, 32), (100, 33)])
def test_result_is_independent_of_position_and_batch_and_repeats_bitwise(qr, plan, m, n):
    A = _rand(31 * m + n, 9, m, n)
    A[4] = A[0]
    A[8] = A[0]
    F, tau, Q = _factor(plan, A)
    for q in (4, 8):
        assert np.array_equal(F[q], F[0]) and np.array_equal(tau[q], tau[0]) and np.array_equal(Q[q], Q[0])
    F1, tau1, Q1 = _factor(plan, A[:1])
    assert np.array_equal(F1[0], F[0]) and np.array_equal(tau1[0], tau[0]) and np.array_equal(Q1[0], Q[0])
    F2, tau2, Q2 = _factor(plan, A)
    assert np.array_equal(F2, F) and np.array_equal(tau2, tau) and np.array_equal(Q2, Q)
    # the fused and the composed least squares as well
    for nrhs in (2, 40):
        Bm = _rand(nrhs, 9, m, nrhs)
        Bm[4] = Bm[0]
        Bm[8] = Bm[0]
        X, _, info = _gels(plan, A, Bm)
        X1, _, _ = _gels(plan, A[:1], Bm[:1])
        X2, _, _ = _gels(plan, A, Bm)
        assert not info.any()
        assert np.array_equal(X[4], X[0]) and np.array_equal(X[8], X[0]) and np.array_equal(X1[0], X[0]) and np.array_equal(X2, X)


@pytest.mark.parametrize("m,n,batch", [(64, 32, 5), (100, 33, 3)])
def test_ormqr_round_trip_and_norms(qr, plan, m, n, batch):
    A = _rand(m + n, batch, m, n)
    F, tau, _ = _factor(plan, A, with_q=False)
    dF, dt = _up(_pack(F)), _up(tau)
    for nrhs in (1, 5, 70):
        Cm = _rand(nrhs, batch, m, nrhs)
        dC = _up(_pack(Cm))
        plan.ormqr_batched("T", dF, m, n, m, m * n, dt, n, dC, nrhs, m, m * nrhs, batch)
        plan.sync()
        Y = _down(dC).transpose(0, 2, 1).copy()
        plan.ormqr_batched("N", dF, m, n, m, m * n, dt, n, dC, nrhs, m, m * nrhs, batch)
        plan.sync()
        Z = _down(dC).transpose(0, 2, 1)
        trip = _nrm(Z - Cm) / _nrm(Cm)
        cn, yn = np.sqrt((Cm * Cm).sum(axis=1)), np.sqrt((Y * Y).sum(axis=1))
        norms = np.abs(yn - cn) / cn
        print(f"batched ormqr {m}x{n} x{batch}, {nrhs} rhs: round trip {trip.max() / EPS:.2f} eps, column norms {norms.max() / EPS:.2f} eps "
              f"(bound {n + 8})")
        assert trip.max() <= (n + 8) * EPS
        assert norms.max() <= (n + 8) * EPS
        # against numpy: the leading n rows of Q^T C are Q_thin^T C
        if nrhs == 5:
            Ql = np.stack([np.linalg.qr(A[q], mode="reduced")[0] for q in range(batch)])
            Rl = np.stack([np.linalg.qr(A[q], mode="r") for q in range(batch)])
            sgn = np.sign(np.diagonal(Rl, axis1=1, axis2=2)) * np.sign(np.diagonal(F[:, :n, :], axis1=1, axis2=2))
            ref = (Ql * sgn[:, None, :]).transpose(0, 2, 1) @ Cm
            assert (_nrm(Y[:, :n, :] - ref) / _nrm(ref)).max() <= 50 * np.linalg.cond(A).max() * EPS


def _gels(plan, A, Bm):
    """returns X (batch, n, nrhs), the residual sums of squares (batch, nrhs), info"""
    batch, m, n = A.shape
    nrhs = Bm.shape[2]
    dA, dtau, dB = _up(_pack(A)), _up(np.zeros((batch, n))), _up(_pack(Bm))
    dinfo = _up(np.full(batch, -9, dtype=np.int32))
    plan.gels_batched(dA, m, n, m, m * n, dtau, n, dB, nrhs, m, m * nrhs, dinfo, batch)
    plan.sync()
    Y = _down(dB).transpose(0, 2, 1)
    return Y[:, :n, :].copy(), (Y[:, n:, :] ** 2).sum(axis=1), _down(dinfo).astype(np.int64)


def _check_ls(A, Bm, X, rss, skip=()):
    """every matrix against numpy.linalg.lstsq; returns the worst multiples of the two bounds"""
    wx = wr = 0.0
    for q in range(A.shape[0]):
        if q in skip:
            continue
        Xn = np.linalg.lstsq(A[q], Bm[q], rcond=None)[0]
        rn = Bm[q] - A[q] @ Xn
        kappa, a2 = np.linalg.cond(A[q]), np.linalg.norm(A[q], 2)
        bound = 50 * (kappa + kappa ** 2 * np.linalg.norm(rn) / (a2 * np.linalg.norm(Xn))) * EPS
        ex = np.linalg.norm(X[q] - Xn) / np.linalg.norm(Xn)
        wx = max(wx, ex / bound)
        assert ex <= bound, (q, ex, bound)
        for j in range(Bm.shape[2]):
            rj = np.linalg.norm(rn[:, j])
            rb = 100 * a2 * np.linalg.norm(Xn[:, j]) * EPS * rj
            er = abs(rss[q, j] - rj * rj)
            if rb > 0:
                wr = max(wr, er / rb)
            assert er <= rb, (q, j, er, rb)
    return wx, wr


@pytest.mark.parametrize("m,n,nrhs,batch,fused", [(5, 3, 1, 6, True), (64, 29, 3, 9, True), (100, 33, 2, 5, True),
                                                  (256, 64, 4, 2, False), (64, 32, 40, 3, False)])
def test_gels_matches_numpy(qr, plan, m, n, nrhs, batch, fused):
    assert fused == (n + nrhs <= 64 and m <= qr.batched_max_rows(n + nrhs))      # the case sits on the route it is meant for
    A = _rand(3 * m + n, batch, m, n)
    Bm = _rand(5 * m + nrhs, batch, m, nrhs)
    X, rss, info = _gels(plan, A, Bm)
    assert not info.any()
    wx, wr = _check_ls(A, Bm, X, rss)
    print(f"batched gels {m}x{n}, {nrhs} rhs x{batch} ({'fused' if fused else 'composed'}): X at {wx:.3f} of its bound, "
          f"residual sums of squares at {wr:.3f} of theirs")


def test_gels_reports_a_singular_matrix_and_solves_the_others(qr, plan):
    m, n, nrhs, batch = 33, 8, 2, 5
    A = _rand(91, batch, m, n)
    A[2, :, 0] = 0.0
    Bm = _rand(92, batch, m, nrhs)
    X, rss, info = _gels(plan, A, Bm)              # (returning at all: the call's status was 0)
    assert list(info) == [0, 0, 1, 0, 0]
    _check_ls(A, Bm, X, rss, skip=(2,))
    # the host twin on the same data: the same info and QR_E_SINGULAR
    At, Bt = _pack(A), _pack(Bm)
    Xh, rh, ih = np.empty((batch, nrhs, n)), np.empty((batch, nrhs)), np.full(batch, -9, dtype=np.intc)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = qr.lib.qr_lstsq_batched(At.ctypes.data_as(dp), m, n, Bt.ctypes.data_as(dp), nrhs, batch, Xh.ctypes.data_as(dp),
                                 rh.ctypes.data_as(dp), ih.ctypes.data_as(ip))
    assert rc == qr.QR_E_SINGULAR
    assert list(ih) == [0, 0, 1, 0, 0]
    _check_ls(A, Bm, Xh.transpose(0, 2, 1), rh ** 2, skip=(2,))
    # the composed route reports it the same way
    B40 = _rand(93, batch, m, 60)
    X40, rss40, info40 = _gels(plan, A, B40)
    assert list(info40) == [0, 0, 1, 0, 0]
    _check_ls(A, B40, X40, rss40, skip=(2,))


def test_host_twins_match_numpy(qr):
    m, n, batch = 20, 6, 11
    A = _rand(206, batch, m, n)
    Q, R = qr.qr_batched(A)
    assert Q.shape == (batch, m, n) and R.shape == (batch, n, n)
    assert (_nrm(A - Q @ R) / _nrm(A)).max() <= (n + 8) * EPS
    assert _nrm(Q.transpose(0, 2, 1) @ Q - np.eye(n)).max() <= (n + 8) * EPS
    assert np.all(np.tril(R, -1) == 0.0)
    Fl, _ = _lapack(A)
    Rl = np.triu(Fl[:, :n, :])
    assert (_nrm(R - Rl) / _nrm(Rl) / (np.linalg.cond(A) * EPS)).max() <= 50
    Bm = _rand(207, batch, m, 3)
    X, resid, info = qr.lstsq_batched(A, Bm)
    assert X.shape == (batch, n, 3) and resid.shape == (batch, 3) and not info.any()
    _check_ls(A, Bm, X, resid ** 2)
