"""-m gpu: column-pivoted QR and rank-deficient least squares (mi355x_qr.h section 4).

There is no reference counterpart (the reference stops at Q and R): the yardsticks are the properties LAPACK dgeqp3 guarantees and a plain
numpy Businger-Golub (exact partial norms at every step, `_businger_golub` below).
"""
import numpy as np
import pytest
import torch

from gpu_util import dev, host, rel, zeros

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
TOL = 100 * np.sqrt(EPS)       # LAPACK keeps a downdated norm while its estimated relative error is below sqrt(eps); 100: margin for the constant


def _businger_golub(A):
    """Householder QR with column pivoting, the partial norms recomputed exactly at every step: (perm, |diag R|)"""
    R = np.array(A, dtype=np.float64)
    m, n = R.shape
    perm = np.arange(n)
    for j in range(n):
        p = j + int(np.argmax(np.linalg.norm(R[j:, j:], axis=0)))
        R[:, [j, p]] = R[:, [p, j]]
        perm[[j, p]] = perm[[p, j]]
        x = R[j:, j]
        s = np.linalg.norm(x)
        if s == 0.0:
            continue
        v = x.copy()
        v[0] += np.copysign(s, x[0])
        v /= np.linalg.norm(v)
        R[j:, j:] -= 2.0 * np.outer(v, v @ R[j:, j:])
    return perm, np.abs(np.diag(R))


def _ints(n):
    t = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def _factor(qr, A, p=None):
    """geqp3 on a plan of its own (or `p`, then queued and not synchronised): (plan, dA, dtau, djpvt)"""
    m, n = A.shape
    if p is None:
        p = qr.Plan(m, n, 0, 0)
    dA, dtau, dj = dev(A), zeros(n, 1), _ints(n)
    p.geqp3(dA, m, n, m, dj, dtau)
    return p, dA, dtau, dj


def _check_factors(qr, p, A, dA, dtau, dj, lda=None, roundtrip=True):
    """properties 1 of the issue; returns (R, jpvt)"""
    m, n = A.shape
    lda = lda or m
    p.sync()
    jp = dj.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(jp), np.arange(n)), "jpvt is not a permutation"
    dQ = zeros(m, n)
    p.applyq(dA, m, n, lda, dtau, dQ, n, m, True)
    p.sync()
    Q = host(dQ)
    F = dA.cpu().numpy().ravel()[: lda * n].reshape(n, lda)[:, :m].T
    assert np.all(np.isfinite(F)) and np.all(np.isfinite(dtau.cpu().numpy()))
    R = np.triu(F[:n])
    e1 = np.linalg.norm(A[:, jp] - Q @ R) / max(np.linalg.norm(A), 1e-300)
    e2 = np.linalg.norm(Q.T @ Q - np.eye(n))
    print(f"geqp3 {m}x{n}: residual {e1:.2e}, orthogonality {e2:.2e}")
    assert e1 < 1e-13, e1
    assert e2 < 1e-13 * n, e2
    if roundtrip:
        rng = np.random.default_rng(m + n)
        Cm = rng.random((m, 3)) - 0.5
        dC = dev(Cm)
        p.ormqr("T", dA, m, n, lda, dtau, dC, 3, m)
        p.sync()
        Y = host(dC)
        assert rel(Y[:n], Q.T @ Cm) < 3e-13
        p.ormqr("N", dA, m, n, lda, dtau, dC, 3, m)
        p.sync()
        e3 = rel(host(dC), Cm)
        assert e3 < 3e-13, e3
    return R, jp


def _check_pivoting(R, full_rank=False):
    """property 2: the diagonal decreases and dominates every trailing partial column norm, to TOL, above the rounding floor"""
    n = R.shape[0]
    d = np.abs(np.diag(R))
    live = d > n * EPS * d[0]
    if full_rank:
        assert live.all(), "a full-rank input must have no excluded row"
    S = np.cumsum((R * R)[::-1], axis=0)[::-1]           # S[j, k] = sum_{i >= j} R[i, k]^2 (R is upper triangular)
    worst = np.inf
    for j in range(n - 1):
        if not live[j]:
            continue
        assert d[j + 1] <= d[j] * (1 + TOL), (j, d[j], d[j + 1])
        best = np.sqrt(S[j, j + 1:].max())
        assert d[j] >= (1 - TOL) * best, (j, d[j], best)
        worst = min(worst, d[j] / best if best > 0 else np.inf)
    print(f"pivoting: smallest d[j] / max trailing partial norm = {worst:.9f}")


def _input(m, n, dist, seed):
    rng = np.random.default_rng(seed)
    A = rng.random((m, n))
    return A - 0.5 if dist == "sym" else A


SHAPES = [(1000, 37), (1000, 300), (2000, 2000), (4096, 4096), (5001, 300), (16384, 256), (65536, 128), (1, 1), (7, 1), (300, 1)]


@pytest.mark.parametrize("dist", ["sym", "pos"])
@pytest.mark.parametrize("m,n", SHAPES)
def test_geqp3_factorisation_and_pivoting(qr, m, n, dist):
    A = _input(m, n, dist, 3 * m + n)
    p, dA, dtau, dj = _factor(qr, A)
    R, jp = _check_factors(qr, p, A, dA, dtau, dj)
    _check_pivoting(R, full_rank=True)
    if (m, n) == (1000, 300):
        perm, dref = _businger_golub(A)
        if not np.array_equal(jp, perm):
            j = int(np.argmax(jp != perm))
            Qj = np.linalg.qr(A[:, perm[:j]])[0] if j else np.zeros((m, 0))
            res = A[:, [jp[j], perm[j]]]
            res = res - Qj @ (Qj.T @ res)
            na, nb = np.linalg.norm(res, axis=0)
            print(f"pivot order differs from Businger-Golub at step {j}: partial norms {na:.17g} / {nb:.17g}")
            assert abs(na - nb) <= TOL * max(na, nb), (j, na, nb)
        else:
            assert np.max(np.abs(np.abs(np.diag(R)) - dref)) < 1e-12 * dref[0]
    p.close()


@pytest.mark.parametrize("m,n,lda,off", [(4096, 1024, 4097, 0), (2049, 700, 2051, 1), (5001, 640, 5003, 1)])
def test_geqp3_on_odd_leading_dimensions_and_misaligned_arrays(qr, m, n, lda, off):
    rng = np.random.default_rng(m + lda)
    A = rng.random((m, n)) - 0.5
    abuf = np.full(lda * n + off, 7.25)
    abuf[off:].reshape(n, lda)[:, :m] = A.T
    dAb = torch.from_numpy(abuf).cuda()
    dA = dAb[off:]
    dtau, dj = zeros(n, 1), _ints(n)
    torch.cuda.synchronize()
    p = qr.Plan(m, n, 0, 0)
    p.geqp3(dA, m, n, lda, dj, dtau)
    p.sync()
    out = dAb.cpu().numpy()
    assert np.array_equal(out[:off], abuf[:off])
    assert np.array_equal(out[off:].reshape(n, lda)[:, m:], abuf[off:].reshape(n, lda)[:, m:]), "rows beyond m are the caller's"
    R, jp = _check_factors(qr, p, A, dA, dtau, dj, lda=lda)
    _check_pivoting(R, full_rank=True)
    p.close()


def _graded(m, n, ratio, seed):
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((m, n)))[0]
    s = ratio ** np.arange(n)
    pi = rng.permutation(n)
    A = np.empty((m, n))
    A[:, pi] = U * s
    return A, s, pi


@pytest.mark.parametrize("m,n,ratio", [(1200, 300, 0.97), (5001, 640, 0.99)])
def test_geqp3_exact_pivot_order_on_graded_orthogonal_columns(qr, m, n, ratio):
    A, s, pi = _graded(m, n, ratio, m)
    p, dA, dtau, dj = _factor(qr, A)
    R, jp = _check_factors(qr, p, A, dA, dtau, dj)
    assert np.array_equal(jp, pi)
    assert np.max(np.abs(np.abs(np.diag(R)) - s)) < 1e-12 * s.max()
    assert p.rank(dA, m, n, m, rcond=0.5) == int(np.sum(s > 0.5 * s[0]))
    p.close()


@pytest.mark.parametrize("kind", ["ones_1e-10", "scaled_1e-7"])
def test_geqp3_cancellation(qr, kind):
    m, n = 1500, 300
    rng = np.random.default_rng(21)
    g, G, u = rng.standard_normal(m), rng.standard_normal((m, n)), rng.random(n)
    A = np.outer(g, np.ones(n)) + 1e-10 * G if kind == "ones_1e-10" else np.outer(g, 1 + u) + 1e-7 * G
    p, dA, dtau, dj = _factor(qr, A)
    R, jp = _check_factors(qr, p, A, dA, dtau, dj)
    _check_pivoting(R)
    d = np.abs(np.diag(R))
    _, dref = _businger_golub(A)
    print(f"cancellation {kind}: d1/d0 = {d[1] / d[0]:.3e}, Businger-Golub {dref[1] / dref[0]:.3e}")
    assert 0.5 <= (d[1] / d[0]) / (dref[1] / dref[0]) <= 2.0
    p.close()


LOW_RANK = [(1500, 400, 100), (3000, 1000, 37), (800, 800, 799)]


def _low_rank(m, n, r):
    rng = np.random.default_rng(m + n + r)
    return rng.standard_normal((m, r)) @ rng.standard_normal((r, n))


@pytest.mark.parametrize("m,n,r", LOW_RANK)
def test_rank_of_low_rank_products(qr, m, n, r):
    A = _low_rank(m, n, r)
    p, dA, dtau, dj = _factor(qr, A)
    got = p.rank(dA, m, n, m)
    d = np.abs(np.diag(host(dA)[:n]))
    print(f"rank {m}x{n} r={r}: d[r-1]/d[0] = {d[r - 1] / d[0]:.2e}, d[r]/d[0] = {d[r] / d[0]:.2e}")
    assert got == r == np.linalg.matrix_rank(A)
    p.close()


def test_rank_full_and_zero(qr):
    m, n = 1000, 300
    A = _input(m, n, "sym", 1)
    p, dA, dtau, dj = _factor(qr, A)
    assert p.rank(dA, m, n, m) == n
    Z = np.zeros((m, n))
    _, dZ, dtz, djz = _factor(qr, Z, p)
    assert p.rank(dZ, m, n, m) == 0
    assert np.array_equal(dtz.cpu().numpy(), np.zeros((1, n)))
    assert np.array_equal(host(dZ), Z)
    assert np.array_equal(np.sort(djz.cpu().numpy()), np.arange(n))
    X, resid, rank, jp = qr.lstsq_pivoted(Z, np.ones((m, 2)))
    assert rank == 0 and np.array_equal(X, np.zeros((n, 2))) and np.allclose(resid, np.sqrt(m), rtol=1e-14)
    p.close()


def _gelsp(qr, A, B, rc):
    m, n = A.shape
    nrhs = B.shape[1]
    p = qr.Plan(m, n, 0, 0)
    dA, dB, dtau, dj, dres = dev(A), dev(B), zeros(n, 1), _ints(n), zeros(nrhs, 1)
    r = p.gelsp(dA, m, n, m, dj, dtau, dB, nrhs, m, rcond=rc, dresid=dres)
    p.sync()
    out = host(dB)[:n], dres.cpu().numpy().ravel(), r, dj.cpu().numpy().astype(np.int64)
    p.close()
    return out


@pytest.mark.parametrize("m,n,r", LOW_RANK[:2])
@pytest.mark.parametrize("nrhs", [3, 17])
def test_gelsp_and_lstsq_pivoted_on_low_rank_matrices(qr, m, n, r, nrhs):
    A = _low_rank(m, n, r)
    rng = np.random.default_rng(nrhs)
    B = rng.random((m, nrhs)) - 0.5
    rc = max(m, n) * EPS
    Xn = np.linalg.lstsq(A, B, rcond=rc)[0]
    rn = np.linalg.norm(A @ Xn - B, axis=0)
    for X, resid, rank, jp in (_gelsp(qr, A, B, rc), qr.lstsq_pivoted(A, B, rcond=rc)):
        assert rank == r
        rh = np.linalg.norm(A @ X - B, axis=0)
        e1, e2 = np.max(np.abs(resid - rh) / rh), np.max(np.abs(resid - rn) / rn)
        print(f"gelsp {m}x{n} r={r} nrhs={nrhs}: resid vs host {e1:.2e}, vs numpy {e2:.2e}")
        assert e1 <= 1e-12 and e2 <= 1e-12
        zero_rows = np.flatnonzero(np.all(X == 0.0, axis=1))
        assert zero_rows.size == n - r and np.array_equal(zero_rows, np.sort(jp[r:]))


@pytest.mark.parametrize("m,n,r", LOW_RANK)
def test_gelsp_consistent_systems(qr, m, n, r):
    A = _low_rank(m, n, r)
    rng = np.random.default_rng(7)
    B = A @ (rng.random((n, 4)) - 0.5)
    rc = max(m, n) * EPS
    for X, resid, rank, jp in (_gelsp(qr, A, B, rc), qr.lstsq_pivoted(A, B, rcond=rc)):
        assert rank == r
        print(f"consistent {m}x{n} r={r}: resid / |b| = {np.max(resid / np.linalg.norm(B, axis=0)):.2e}")
        assert np.all(resid <= 1e-11 * np.linalg.norm(B, axis=0))
        assert np.all(np.linalg.norm(A @ X - B, axis=0) <= 1e-11 * np.linalg.norm(B, axis=0))


def _cond_matrix(m, n, cond, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * np.logspace(0, -np.log10(cond), n)) @ V.T


def _check(A, B, X, resid, kappa, consistent=False):
    """the bound of tests/test_gpu_lstsq.py: X against LAPACK's to (kappa + kappa^2 ||r|| / (||A|| ||X||)) eps, times 50"""
    Xn = np.linalg.lstsq(A, B, rcond=None)[0]
    rn = np.linalg.norm(A @ Xn - B, axis=0)
    bound = kappa + kappa ** 2 * np.linalg.norm(rn) / (np.linalg.norm(A, 2) * np.linalg.norm(Xn))
    assert rel(X, Xn) <= 50 * bound * EPS, (rel(X, Xn), bound)
    if consistent:
        assert np.all(resid <= 1e-11 * np.linalg.norm(B, axis=0))
    else:
        assert np.max(np.abs(resid - rn) / rn) <= 1e-12


@pytest.mark.parametrize("case", ["well", "cond1e6", "wide_rhs"])
def test_gelsp_on_full_rank_inputs_matches_numpy(qr, case):
    rng = np.random.default_rng(11)
    consistent = case == "cond1e6"
    if case == "well":
        A, nrhs = rng.random((2000, 300)) - 0.5, 5
    elif case == "cond1e6":
        A, nrhs = _cond_matrix(1500, 200, 1e6, 1), 3
    else:
        A, nrhs = rng.random((3000, 256)) - 0.5, 20
    m, n = A.shape
    B = A @ (rng.random((n, nrhs)) - 0.5) if consistent else rng.random((m, nrhs)) - 0.5
    kappa = np.linalg.cond(A)
    for X, resid, rank, jp in (_gelsp(qr, A, B, None), qr.lstsq_pivoted(A, B)):
        assert rank == n
        _check(A, B, X, resid, kappa, consistent)


def test_geqp3_is_deterministic(qr):
    m, n = 8192, 512
    A = _input(m, n, "pos", 13)
    p = qr.Plan(m, n, 0, 0)
    outs = []
    for _ in range(2):
        _, dA, dtau, dj = _factor(qr, A, p)
        p.sync()
        outs.append((dA.cpu().numpy(), dtau.cpu().numpy(), dj.cpu().numpy()))
    p.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_geqp3_back_to_back_on_one_plan(qr):
    m, n = 4000, 512
    A1, A2 = _input(m, n, "pos", 1), _input(m, n, "sym", 2)
    p = qr.Plan(m, n, 0, 0)
    f1 = _factor(qr, A1, p)
    f2 = _factor(qr, A2, p)
    for A, f in ((A1, f1), (A2, f2)):
        R, jp = _check_factors(qr, p, A, f[1], f[2], f[3])
        _check_pivoting(R, full_rank=True)
    p.close()


def test_geqrf_after_a_pivoted_factorisation_equals_a_fresh_plan(qr):
    m, n = 4096, 1024
    A = _input(m, n, "sym", 5)
    p = qr.Plan(m, n, 0, 0)
    _factor(qr, A, p)
    p.sync()
    res = []
    for plan in (p, qr.Plan(m, n, 0, 0)):
        dA, dtau = dev(A), zeros(n, 1)
        plan.geqrf(dA, m, n, m, dtau)
        plan.sync()
        res.append((dA.cpu().numpy(), dtau.cpu().numpy()))
        plan.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_qr_pivoted_host_wrapper(qr):
    A = _input(700, 90, "pos", 4)
    Q, R, jp = qr.qr_pivoted(A)
    assert Q.shape == (700, 90) and R.shape == (90, 90)
    assert rel(Q @ R, A[:, jp]) < 1e-13
    assert np.all(np.diff(np.abs(np.diag(R))) <= TOL * np.abs(R[0, 0]))
