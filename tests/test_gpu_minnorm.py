"""-m gpu: minimum-norm solutions (mi355x_qr.h section 5) against numpy / LAPACK.

qr_solve_rt_dev has a backward error below n eps on both sides of its 64-right-hand-side threshold (substitution satisfies
|dT| <= gamma_n |T| in any summation order and gamma_n ~ n eps / 2: the bound has a factor 2 of slack by construction) and undoes a
product with R^T to 50 kappa(R) eps.  qr_transpose_dev is a copy: exact.  qr_gels_t_dev, qr_minnorm_dev (with and without a prebuilt T),
qr_gels_wide_dev and qr.lstsq_minnorm match numpy.linalg.lstsq's minimum-norm solution to 50 kappa(A) eps (the factor of
test_gpu_lstsq._check; the residual term is zero, the system is consistent) and leave a residual below n eps ||A|| ||X||.
"""
import numpy as np
import pytest
import torch

from gpu_util import dev, host, rel, zeros

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def _rand_dev(rows, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.rand((cols, rows), dtype=torch.float64, device="cuda", generator=g) - 0.5
    torch.cuda.synchronize()
    return t


def _cond_matrix(m, n, cond, seed):
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * np.logspace(0, -np.log10(cond), n)) @ V.T


# ------------------------------------------------------------------------------------------------
# qr_solve_rt_dev
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1000, 4096, 16384])
def test_solve_rt_backward_error(qr, n):
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
        p.solve_rt(dA, n, n, X, nrhs, n)
        p.sync()
        berr = (torch.linalg.norm(R.T @ X.T - B.T) / (nR * torch.linalg.norm(X))).item()
        print(f"solve_rt n={n} nrhs={nrhs}: backward error {berr:.3e} (bound {n * EPS:.3e})")
        assert berr <= n * EPS, (nrhs, berr)
    p.close()


def test_solve_rt_ill_conditioned(qr):
    n = 1000
    A = _cond_matrix(n, n, 1e10, 3)
    p = qr.Plan(n, n, 0, 0)
    dA, dtau = dev(A), zeros(n, 1)
    p.geqrf(dA, n, n, n, dtau)
    p.sync()
    R = np.triu(host(dA)[:n])
    kappa = np.linalg.cond(R)
    assert kappa > 1e9
    for nrhs in (1, 16, 80):
        B = np.random.default_rng(nrhs).random((n, nrhs))
        dB = dev(B)
        p.solve_rt(dA, n, n, dB, nrhs, n)
        p.sync()
        X = host(dB)
        berr = np.linalg.norm(R.T @ X - B) / (np.linalg.norm(R) * np.linalg.norm(X))
        back = rel(R.T @ X, B)
        print(f"solve_rt cond 1e10 nrhs={nrhs}: backward error {berr:.3e} (bound {n * EPS:.3e}), R^T X against B {back:.3e} "
              f"(bound {50 * kappa * EPS:.3e})")
        assert berr <= n * EPS, (nrhs, berr)
        assert back <= 50 * kappa * EPS, (nrhs, back)
    p.close()


@pytest.mark.parametrize("n", [64, 1000])
def test_solve_rt_then_product_recovers_b(qr, n):
    A = np.random.default_rng(n).random((n, n)) - 0.5
    p = qr.Plan(n, n, 0, 0)
    dA, dtau = dev(A), zeros(n, 1)
    p.geqrf(dA, n, n, n, dtau)
    p.sync()
    R = np.triu(host(dA)[:n])
    kappa = np.linalg.cond(R)
    for nrhs in (1, 4, 17, 64, 65):
        B = np.random.default_rng(nrhs).random((n, nrhs)) - 0.5
        dB = dev(B)
        p.solve_rt(dA, n, n, dB, nrhs, n)
        p.sync()
        back = rel(R.T @ host(dB), B)
        assert back <= 50 * kappa * EPS, (nrhs, back, kappa)
    p.close()


# ------------------------------------------------------------------------------------------------
# qr_transpose_dev
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(4096, 4096), (300, 5001), (5001, 300), (1, 777), (65, 63)])
def test_transpose_is_exact_on_odd_leading_dimensions_and_misaligned_arrays(qr, rows, cols):
    rng = np.random.default_rng(rows + cols)
    S = rng.random((rows, cols))
    lds, ldd, off = rows + 3 - rows % 2, cols + 3 - cols % 2, 1        # odd leading dimensions, bases one double off
    assert lds % 2 == 1 and ldd % 2 == 1
    sbuf = np.full(lds * cols + off, 7.25)
    sbuf[off:].reshape(cols, lds)[:, :rows] = S.T
    dbuf = np.full(ldd * rows + off, -3.5)
    dS, dD = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf).cuda()
    torch.cuda.synchronize()
    p = qr.Plan(64, 32, 0, 0)                  # the sizes are not bounded by the plan's
    p.transpose(dS[off:], rows, cols, lds, dD[off:], ldd)
    p.sync()
    out = dD.cpu().numpy()
    assert np.array_equal(dS.cpu().numpy(), sbuf), "the source is read only"
    assert np.array_equal(out[:off], dbuf[:off])
    Dm = out[off:].reshape(rows, ldd)          # column i of D (cols x rows) = row i of S
    assert np.array_equal(Dm[:, :cols], S)
    assert np.array_equal(Dm[:, cols:], dbuf[off:].reshape(rows, ldd)[:, cols:]), "rows beyond cols are the caller's"
    # even leading dimensions and aligned bases
    dS2, dD2 = dev(S), zeros(cols, rows)
    p.transpose(dS2, rows, cols, rows, dD2, cols)
    p.sync()
    assert np.array_equal(host(dD2), S.T)
    p.close()


# ------------------------------------------------------------------------------------------------
# minimum norm against numpy
# ------------------------------------------------------------------------------------------------
def _case(name):
    """(At, nrhs): the tall generators of test_gpu_lstsq.py; the wide system is At^T"""
    rng = np.random.default_rng(11)
    if name == "well":
        return rng.random((2000, 300)) - 0.5, 5
    if name == "cond1e6":
        return _cond_matrix(1500, 200, 1e6, 1), 3
    if name == "cond1e10":
        return _cond_matrix(1500, 200, 1e10, 2), 3
    if name == "wide_rhs":
        return rng.random((3000, 256)) - 0.5, 20
    if name == "tall_skinny":                   # (an addition: the VALU route of qr_ormqr_dev('N'), m >= 16 n and <= 4 right-hand sides)
        return rng.random((8192, 256)) - 0.5, 2
    assert name == "square1024"
    return rng.random((1024, 1024)) - 0.5, 2


def _check(name, Aw, B, X, Xn, kappa):
    nbig = Aw.shape[1]
    e1 = rel(X, Xn)
    e2 = np.linalg.norm(Aw @ X - B) / (np.linalg.norm(Aw, 2) * np.linalg.norm(X))
    print(f"{name}: |X - X_numpy| / |X_numpy| = {e1:.3e} (bound {50 * kappa * EPS:.3e}), residual {e2:.3e} (bound {nbig * EPS:.3e})")
    assert e1 <= 50 * kappa * EPS, (name, e1, kappa)
    assert e2 <= nbig * EPS, (name, e2)


def _padded_rhs(B, rows):
    """B on top of garbage rows: the tail rows of dB are ignored on entry"""
    Bp = np.full((rows, B.shape[1]), 123.456)
    Bp[:B.shape[0]] = B
    return Bp


@pytest.mark.parametrize("case", ["well", "cond1e6", "cond1e10", "wide_rhs", "square1024", "tall_skinny"])
def test_minimum_norm_matches_numpy(qr, case):
    At, nrhs = _case(case)
    nbig, msmall = At.shape                     # At: nbig x msmall (tall); the wide system Aw X = B is msmall x nbig
    Aw = np.ascontiguousarray(At.T)
    B = np.random.default_rng(17).random((msmall, nrhs)) - 0.5
    Xn = np.linalg.lstsq(Aw, B, rcond=None)[0]
    kappa = np.linalg.cond(At)
    p = qr.Plan(nbig, msmall, 0, 0)
    nb = p.nb

    # qr_gels_t_dev
    dA, dtau, dB = dev(At), zeros(msmall, 1), dev(_padded_rhs(B, nbig))
    p.gels_t(dA, nbig, msmall, nbig, dtau, dB, nrhs, nbig)
    p.sync()
    X_t = host(dB)
    _check(case + " gels_t", Aw, B, X_t, Xn, kappa)

    # qr_minnorm_dev on factors that already exist, T rebuilt panel by panel: the same launches as gels_t's second half
    dA2, dtau2 = dev(At), zeros(msmall, 1)
    p.geqrf(dA2, nbig, msmall, nbig, dtau2)
    dB2 = dev(_padded_rhs(B, nbig))
    p.minnorm(dA2, nbig, msmall, nbig, dtau2, dB2, nrhs, nbig)
    p.sync()
    X_f = host(dB2)
    _check(case + " minnorm", Aw, B, X_f, Xn, kappa)
    assert np.array_equal(X_f, X_t), "factor once, solve many: the same result as qr_gels_t_dev"

    # ... and with a prebuilt T
    dT = zeros(nb, msmall)
    p.build_t(dA2, nbig, msmall, nbig, dtau2, dT, nb)
    dB3 = dev(_padded_rhs(B, nbig))
    p.minnorm(dA2, nbig, msmall, nbig, dtau2, dB3, nrhs, nbig, dT=dT, ldt=nb)
    p.sync()
    _check(case + " minnorm with T", Aw, B, host(dB3), Xn, kappa)

    # qr_gels_wide_dev: the wide matrix as the caller holds it
    dW, dF, dtau4, dB4 = dev(Aw), zeros(nbig, msmall), zeros(msmall, 1), dev(_padded_rhs(B, nbig))
    p.gels_wide(dW, msmall, nbig, msmall, dF, nbig, dtau4, dB4, nrhs, nbig)
    p.sync()
    X_w = host(dB4)
    _check(case + " gels_wide", Aw, B, X_w, Xn, kappa)
    assert np.array_equal(host(dW), Aw), "the wide matrix is not modified"
    assert np.array_equal(host(dF), host(dA)), "dF = the factors of the transpose"
    assert np.array_equal(X_w, X_t)
    p.close()

    # host pointers
    X_h = qr.lstsq_minnorm(Aw, B)
    assert X_h.shape == (nbig, nrhs)
    _check(case + " lstsq_minnorm", Aw, B, X_h, Xn, kappa)
    x1 = qr.lstsq_minnorm(Aw, B[:, 0])
    assert x1.shape == (nbig,) and np.array_equal(x1, qr.lstsq_minnorm(Aw, B[:, :1])[:, 0])


def test_gels_wide_keeps_its_input_and_its_factors_solve_again(qr):
    rng = np.random.default_rng(23)
    m, n, nrhs = 300, 2500, 3
    Aw = rng.random((m, n)) - 0.5
    B1, B2 = rng.random((m, nrhs)), rng.random((m, 7)) - 0.5
    kappa = np.linalg.cond(Aw)
    p = qr.Plan(n, m, 0, 0)
    dW, dF, dtau, dB = dev(Aw), zeros(n, m), zeros(m, 1), dev(_padded_rhs(B1, n))
    p.gels_wide(dW, m, n, m, dF, n, dtau, dB, nrhs, n)
    p.sync()
    assert np.array_equal(host(dW), Aw)
    _check("gels_wide", Aw, B1, host(dB), np.linalg.lstsq(Aw, B1, rcond=None)[0], kappa)
    dB2 = dev(_padded_rhs(B2, n))
    p.minnorm(dF, n, m, n, dtau, dB2, 7, n)
    p.sync()
    _check("minnorm on gels_wide's factors", Aw, B2, host(dB2), np.linalg.lstsq(Aw, B2, rcond=None)[0], kappa)
    p.close()


@pytest.mark.parametrize("m,n,lda,ldf,ldb,off", [(700, 2049, 701, 2051, 2053, 1), (129, 1000, 131, 1001, 1003, 1)])
def test_gels_wide_on_odd_leading_dimensions_and_misaligned_arrays(qr, m, n, lda, ldf, ldb, off):
    rng = np.random.default_rng(m + n)
    Aw = rng.random((m, n)) - 0.5
    nrhs = 5
    B = rng.random((m, nrhs)) - 0.5
    abuf = np.full(lda * n + off, 7.25)
    abuf[off:].reshape(n, lda)[:, :m] = Aw.T
    fbuf = np.full(ldf * m + off, -1.5)
    bbuf = np.full(ldb * nrhs + off, -3.5)
    bbuf[off:].reshape(nrhs, ldb)[:, :m] = B.T
    dAb, dFb, dBb = (torch.from_numpy(x).cuda() for x in (abuf, fbuf, bbuf))
    dtau = zeros(m, 1)
    torch.cuda.synchronize()
    p = qr.Plan(n, m, 0, 0)
    p.gels_wide(dAb[off:], m, n, lda, dFb[off:], ldf, dtau, dBb[off:], nrhs, ldb)
    p.sync()
    assert np.array_equal(dAb.cpu().numpy(), abuf), "the wide matrix and its padding are untouched"
    fout = dFb.cpu().numpy()
    assert np.array_equal(fout[:off], fbuf[:off])
    assert np.array_equal(fout[off:].reshape(m, ldf)[:, n:], fbuf[off:].reshape(m, ldf)[:, n:]), "rows beyond n of dF are the caller's"
    bout = dBb.cpu().numpy()
    assert np.array_equal(bout[:off], bbuf[:off])
    Bo = bout[off:].reshape(nrhs, ldb)
    assert np.array_equal(Bo[:, n:], bbuf[off:].reshape(nrhs, ldb)[:, n:]), "rows beyond n of dB are the caller's"
    _check("gels_wide odd ld", Aw, B, Bo[:, :n].T, np.linalg.lstsq(Aw, B, rcond=None)[0], np.linalg.cond(Aw))
    # R of the factors = R of numpy's QR of A^T up to signs
    Rf = np.triu(fout[off:].reshape(m, ldf)[:, :m].T)
    Rn = np.linalg.qr(Aw.T, mode="r")
    assert rel(np.abs(Rf), np.abs(Rn)) < 1e-12
    p.close()


def test_lstsq_minnorm_zero_row_is_singular(qr):
    A = np.random.default_rng(5).random((40, 300))
    A[7, :] = 0.0
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_minnorm(A, np.ones(40))
    assert ei.value.status == qr.QR_E_SINGULAR


def _gels_t(p, At, B):
    nbig, msmall = At.shape
    dA, dtau, dB = dev(At), zeros(msmall, 1), dev(_padded_rhs(B, nbig))
    p.gels_t(dA, nbig, msmall, nbig, dtau, dB, B.shape[1], nbig)
    return dA, dB, dtau


def test_gels_t_back_to_back_on_one_plan_without_sync(qr):
    rng = np.random.default_rng(9)
    nbig, msmall, nrhs = 4000, 512, 4
    A1, A2 = rng.random((nbig, msmall)), rng.random((nbig, msmall)) - 0.5
    B1, B2 = rng.random((msmall, nrhs)), rng.random((msmall, nrhs))
    p = qr.Plan(nbig, msmall, 0, 0)
    d1 = _gels_t(p, A1, B1)
    d2 = _gels_t(p, A2, B2)
    p.sync()
    for At, B, d in ((A1, B1, d1), (A2, B2, d2)):
        _check("back to back", At.T, B, host(d[1]), np.linalg.lstsq(At.T, B, rcond=None)[0], np.linalg.cond(At))
    p.close()


def test_minimum_norm_is_deterministic(qr):
    rng = np.random.default_rng(13)
    At, B = rng.random((8192, 512)), rng.random((512, 3))
    p = qr.Plan(8192, 512, 0, 0)
    outs = []
    for _ in range(2):
        d = _gels_t(p, At, B)
        p.sync()
        outs.append(host(d[1]))
    p.close()
    assert np.array_equal(outs[0], outs[1])
    n = 4096
    p = qr.Plan(n, n, 0, 0)
    dA, dtau = zeros(n, n), zeros(n, 1)
    p.fill_uniform(dA, n, n, n, seed=5)
    p.geqrf(dA, n, n, n, dtau)
    for nrhs in (4, 100):                       # both routes of qr_solve_rt_dev
        Bd = _rand_dev(n, nrhs, nrhs)
        X1, X2 = Bd.clone(), Bd.clone()
        torch.cuda.synchronize()
        p.solve_rt(dA, n, n, X1, nrhs, n)
        p.solve_rt(dA, n, n, X2, nrhs, n)
        p.sync()
        assert torch.equal(X1, X2)
    p.close()
