"""-m gpu: the least-squares solve (mi355x_qr.h section 3) against the library's own explicit Q and against numpy / LAPACK.

qr_ormqr_dev('T') = Q^T C with Q formed by qr_applyq_dev (identity start), ormqr('N') undoes it, and ormqr('N') with a prebuilt T
equals qr_applyq_dev -- with and without T, on both sides of the VALU / MFMA thresholds (ormqr: up to 4 right-hand sides on tall
matrices; solve_r: up to 64).  qr_solve_r_dev has a backward error below n eps.  qr_gels_dev and qr_lstsq match numpy.linalg.lstsq to c kappa(A) eps.
"""
import numpy as np
import pytest
import torch

from gpu_util import dev, host, rel, zeros

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NRHS = (1, 3, 4, 5, 16, 17, 33, 64, 300)


def _trel(a, b):
    return (torch.linalg.norm(a - b) / torch.linalg.norm(b)).item()


def _rand_dev(rows, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.rand((cols, rows), dtype=torch.float64, device="cuda", generator=g) - 0.5
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("m,n", [(1000, 37), (4096, 4096), (5001, 300), (16384, 256), (65536, 128)])
def test_ormqr_against_explicit_q(qr, m, n):
    p = qr.Plan(m, n, 0, 0)
    nb = p.nb
    dA, dtau = zeros(m, n), zeros(n, 1)
    p.fill_uniform(dA, m, m, n, seed=m + n)
    p.geqrf(dA, m, n, m, dtau)
    dT = zeros(nb, n)
    p.build_t(dA, m, n, m, dtau, dT, nb)
    q = m if m <= 5001 else n                  # the whole m x m Q where it fits, else the thin one (the first n rows of Q^T C)
    dQ = zeros(m, q)
    p.applyq(dA, m, n, m, dtau, dQ, q, m, True)
    p.sync()
    Q = dQ.T                                   # m x q
    worst = 0.0
    for nrhs in NRHS:
        C = _rand_dev(m, nrhs, nrhs)
        ref = Q.T @ C.T                        # q x nrhs
        for T, ldt in ((None, 0), (dT, nb)):
            Y = C.clone()
            torch.cuda.synchronize()
            p.ormqr("T", dA, m, n, m, dtau, Y, nrhs, m, dT=T, ldt=ldt)
            p.sync()
            e1 = _trel(Y.T[:q], ref)
            p.ormqr("N", dA, m, n, m, dtau, Y, nrhs, m, dT=T, ldt=ldt)
            p.sync()
            e2 = _trel(Y, C)
            worst = max(worst, e1, e2)
            assert e1 < 3e-13, (nrhs, T is not None, e1)
            assert e2 < 3e-13, (nrhs, T is not None, e2)
        Z1, Z2 = C.clone(), C.clone()
        torch.cuda.synchronize()
        p.applyq(dA, m, n, m, dtau, Z1, nrhs, m, False)
        p.ormqr("N", dA, m, n, m, dtau, Z2, nrhs, m, dT=dT, ldt=nb)
        p.sync()
        e3 = _trel(Z2, Z1)
        worst = max(worst, e3)
        assert e3 < 3e-13, (nrhs, e3)
    print(f"ormqr {m}x{n}: worst relative difference {worst:.2e}")
    p.close()


@pytest.mark.parametrize("m,n,lda,ldc,off", [(4096, 1024, 4097, 4099, 0), (4096, 1024, 4100, 4101, 1), (2049, 700, 2051, 2049, 0),
                                             (5001, 640, 5001, 5003, 1), (8001, 300, 8003, 8005, 1)])
def test_ormqr_on_odd_leading_dimensions_and_misaligned_arrays(qr, m, n, lda, ldc, off):
    """the arrays test_geqrf_dev_on_odd_leading_dimensions_and_misaligned_arrays factors: V read in place from them, C at an odd offset
    with its own odd leading dimension; nothing outside the m x nrhs block is written"""
    rng = np.random.default_rng(m + lda)
    A = rng.random((m, n))
    abuf = np.full(lda * n + off, 7.25)
    abuf[off:].reshape(n, lda)[:, :m] = A.T
    dAb = torch.from_numpy(abuf).cuda()
    dA = dAb[off:]
    dtau = zeros(n, 1)
    torch.cuda.synchronize()
    p = qr.Plan(m, n, 0, 0)
    p.geqrf(dA, m, n, lda, dtau)
    dQ = zeros(m, m)
    p.applyq(dA, m, n, lda, dtau, dQ, m, m, True)
    p.sync()
    Q = host(dQ)
    for nrhs in (1, 4, 5, 17, 64):
        Cm = rng.random((m, nrhs))
        cbuf = np.full(ldc * nrhs + off, -3.5)
        cbuf[off:].reshape(nrhs, ldc)[:, :m] = Cm.T
        dCb = torch.from_numpy(cbuf).cuda()
        torch.cuda.synchronize()
        p.ormqr("T", dA, m, n, lda, dtau, dCb[off:], nrhs, ldc)
        p.sync()
        out = dCb.cpu().numpy()
        assert np.array_equal(out[:off], cbuf[:off])
        Cout = out[off:].reshape(nrhs, ldc)
        assert np.array_equal(Cout[:, m:], cbuf[off:].reshape(nrhs, ldc)[:, m:]), "rows beyond m are the caller's"
        assert rel(Cout[:, :m].T, Q.T @ Cm) < 3e-13, nrhs
    p.close()


def _factored(qr, A):
    m, n = A.shape
    p = qr.Plan(m, n, 0, 0)
    dA, dtau = dev(A), zeros(n, 1)
    p.geqrf(dA, m, n, m, dtau)
    p.sync()
    return p, dA, dtau


@pytest.mark.parametrize("n", [64, 1000, 4096, 16384])
def test_solve_r_backward_error(qr, n):
    p = qr.Plan(n, n, 0, 0)
    dA, dtau = zeros(n, n), zeros(n, 1)
    p.fill_uniform(dA, n, n, n, seed=n)
    p.geqrf(dA, n, n, n, dtau)
    p.sync()
    R = torch.triu(dA.T[:n, :n])
    nR = torch.linalg.norm(R).item()
    for nrhs in (1, 4, 17, 64, 65):
        B = _rand_dev(n, nrhs, 7 * nrhs)
        X = B.clone()
        torch.cuda.synchronize()
        p.solve_r(dA, n, n, X, nrhs, n)
        p.sync()
        berr = (torch.linalg.norm(R @ X.T - B.T) / (nR * torch.linalg.norm(X))).item()
        assert berr <= n * EPS, (nrhs, berr)
    p.close()


def _cond_matrix(m, n, cond, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * np.logspace(0, -np.log10(cond), n)) @ V.T


def test_solve_r_ill_conditioned(qr):
    n = 1000
    A = _cond_matrix(n, n, 1e10, 3)
    p, dA, dtau = _factored(qr, A)
    R = np.triu(host(dA)[:n])
    assert np.linalg.cond(R) > 1e9
    for nrhs in (1, 16, 80):
        B = np.random.default_rng(nrhs).random((n, nrhs))
        dB = dev(B)
        p.solve_r(dA, n, n, dB, nrhs, n)
        X = host(dB)
        assert np.linalg.norm(R @ X - B) / (np.linalg.norm(R) * np.linalg.norm(X)) <= n * EPS
    p.close()


def _gels(qr, A, B, p=None):
    """host result of qr_gels_dev on a plan of its own; on a given plan: the device buffers (dA, dB, dtau), queued and not synchronised"""
    m, n = A.shape
    own = p is None
    if own:
        p = qr.Plan(m, n, 0, 0)
    dA, dB, dtau = dev(A), dev(B), zeros(n, 1)
    p.gels(dA, m, n, m, dtau, dB, B.shape[1], m)
    if not own:
        return dA, dB, dtau
    p.sync()
    p.close()
    return host(dB)


def _numpy_ls(A, B):
    X = np.linalg.lstsq(A, B, rcond=None)[0] if A.shape[0] != A.shape[1] else np.linalg.solve(A, B)
    return X, np.linalg.norm(A @ X - B, axis=0)


def _check(A, B, X, resid, kappa, consistent=False):
    """X against LAPACK's to the least-squares perturbation bound (kappa + kappa^2 ||r|| / (||A|| ||X||)) eps, times 50"""
    Xn, rn = _numpy_ls(A, B)
    bound = kappa + kappa ** 2 * np.linalg.norm(rn) / (np.linalg.norm(A, 2) * np.linalg.norm(Xn))
    assert rel(X, Xn) <= 50 * bound * EPS, (rel(X, Xn), bound)
    if consistent:
        assert np.all(resid <= 1e-11 * np.linalg.norm(B, axis=0))
    else:
        assert np.max(np.abs(resid - rn) / rn) <= 1e-12


@pytest.mark.parametrize("case", ["well", "cond1e6", "cond1e10", "consistent", "square4096", "c1", "wide_rhs"])
def test_gels_and_lstsq_match_numpy(qr, oracle, case):
    rng = np.random.default_rng(11)
    consistent = case in ("cond1e6", "cond1e10", "consistent", "square4096")
    if case == "well":
        A, nrhs = rng.random((2000, 300)) - 0.5, 5
    elif case == "cond1e6":
        A, nrhs = _cond_matrix(1500, 200, 1e6, 1), 3
    elif case == "cond1e10":
        A, nrhs = _cond_matrix(1500, 200, 1e10, 2), 3
    elif case == "consistent":
        A, nrhs = rng.random((1500, 400)), 2
    elif case == "square4096":
        A, nrhs = rng.random((4096, 4096)) - 0.5, 1
    elif case == "c1":
        A, nrhs = oracle.fill_rand(512, 128), 1
    else:
        A, nrhs = rng.random((3000, 256)) - 0.5, 20
    m, n = A.shape
    if consistent:
        Xt = rng.random((n, nrhs)) - 0.5
        B = A @ Xt
    else:
        B = rng.random((m, nrhs)) - 0.5
    kappa = np.linalg.cond(A)
    Bo = _gels(qr, A, B)
    X, resid = Bo[:n], np.linalg.norm(Bo[n:], axis=0)
    _check(A, B, X, resid, kappa, consistent)
    Xh, rh = qr.lstsq(A, B)
    _check(A, B, Xh, rh, kappa, consistent)
    if case == "consistent":
        assert rel(X, Xt) <= 50 * kappa * EPS and rel(Xh, Xt) <= 50 * kappa * EPS
    if nrhs == 1:
        x1, r1 = qr.lstsq(A, B[:, 0])
        assert x1.shape == (n,) and np.array_equal(x1, Xh[:, 0]) and r1 == rh[0]


def test_lstsq_zero_column_is_singular(qr):
    A = np.random.default_rng(5).random((300, 40))
    A[:, 7] = 0.0
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq(A, np.ones(300))
    assert ei.value.status == qr.QR_E_SINGULAR


def test_gels_back_to_back_on_one_plan_without_sync(qr):
    rng = np.random.default_rng(9)
    m, n, nrhs = 4000, 512, 4
    A1, A2 = rng.random((m, n)), rng.random((m, n)) - 0.5
    B1, B2 = rng.random((m, nrhs)), rng.random((m, nrhs))
    p = qr.Plan(m, n, 0, 0)
    d1 = _gels(qr, A1, B1, p)
    d2 = _gels(qr, A2, B2, p)
    p.sync()
    for A, B, d in ((A1, B1, d1), (A2, B2, d2)):
        Bo = host(d[1])
        _check(A, B, Bo[:n], np.linalg.norm(Bo[n:], axis=0), np.linalg.cond(A))
    p.close()


def test_gels_is_deterministic(qr):
    rng = np.random.default_rng(13)
    A, B = rng.random((8192, 512)), rng.random((8192, 3))
    p = qr.Plan(8192, 512, 0, 0)
    outs = []
    for _ in range(2):
        d = _gels(qr, A, B, p)
        p.sync()
        outs.append(host(d[1]))
    p.close()
    assert np.array_equal(outs[0], outs[1])
