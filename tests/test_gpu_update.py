"""-m gpu: the row-append update (mi355x_qr.h section 6) against numpy / LAPACK.

qr_tpqrt_dev: the Gram identity R'^T R' = R^T R + B^T B to n eps, R' against LAPACK's QR of the stacked matrix to 50 kappa eps, R's strict
lower triangle untouched, an exactly zero column of B stays zero, R = 0 on entry, bitwise-equal repeats.  qr_tpmqrt_dev: 'N' undoes 'T',
'T' keeps column norms, Q'^T [R ; B] = [R' ; 0].  The accumulator and qr_lstsq_chunked against numpy.linalg.lstsq to the bound of
test_gpu_lstsq._check.

Two places where the cases are written differently from a literal reading of their specification:
  * a block of more than qr_tpqrt_max_rows() rows (the case n = 1000, p = 300 at a limit of 256) is fed to qr_tpqrt_dev block by block,
    as the header prescribes; the checks on R' are those of one call, the checks on V and T run per block;
  * the second accumulator case lists chunks of (P + 1, 599, 600, 1, 1200 - P) rows, which is 2401 of the 3000: the remaining 599 rows
    are pushed as one more chunk, so that rows() is 3000 and the solution is the whole matrix's.
"""
import functools

import numpy as np
import pytest
import torch

from gpu_util import dev, host, rel, zeros
from test_gpu_lstsq import _check, _cond_matrix

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = 7.25
TW = 32                       # QR_TPQRT_PANEL


def _P(qr):
    return qr.tpqrt_max_rows()


def _shape(qr, n, p):
    return n, (_P(qr) if p == "P" else p)


CASES = [(33, 1), (96, 7), (200, 37), (600, "P"), (1000, 300)]


@functools.lru_cache(maxsize=None)
def _inputs(n, p):
    """R = the triangle of numpy's QR of a random 2n x n matrix, B uniform in [-0.5, 0.5); computed once per shape, never modified"""
    rng = np.random.default_rng(1000 * n + p)
    R = np.triu(np.linalg.qr(rng.random((2 * n, n)) - 0.5, mode="r"))
    B = rng.random((p, n)) - 0.5
    R.setflags(write=False)
    B.setflags(write=False)
    return R, B


def _strided(A, ld, off, fill):
    """the column-major image of A at leading dimension ld, `off` doubles into a buffer filled with `fill`: (whole buffer, view at off)"""
    m, n = A.shape
    buf = np.full(ld * n + off, fill)
    buf[off:].reshape(n, ld)[:, :m] = A.T
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return t, t[off:]


def _unstrided(t, m, n, ld, off):
    torch.cuda.synchronize()
    return np.asfortranarray(t.cpu().numpy()[off:].reshape(n, ld)[:, :m].T)


def _tpqrt(qr, plan, R, B, off=1):
    """qr_tpqrt_dev on odd leading dimensions and a base one double off, block by block above the row limit.
    Returns (dR contents n x n with whatever lies below the diagonal, V p x n, [T per block], the device buffers)"""
    n, p = R.shape[0], B.shape[0]
    ldr, ldb, P = (n + 2) | 1, (p + 2) | 1, _P(qr)
    Rin = np.triu(R) + np.tril(np.full((n, n), SENTINEL), -1)
    tR, dR = _strided(Rin, ldr, off, -3.5)
    tB, dB = _strided(B, ldb, off, -3.5)
    Ts = []
    for r0 in range(0, p, P):
        dT = zeros(TW, n)
        plan.tpqrt(dR, n, ldr, dB[r0:], min(P, p - r0), ldb, dT, TW)
        Ts.append(dT)
    plan.sync()
    Rout, V = _unstrided(tR, n, n, ldr, off), _unstrided(tB, p, n, ldb, off)
    # nothing outside the two blocks is written
    assert np.all(tR.cpu().numpy()[off:].reshape(n, ldr)[:, n:] == -3.5) and np.all(tB.cpu().numpy()[off:].reshape(n, ldb)[:, p:] == -3.5)
    assert np.all(tR.cpu().numpy()[:off] == -3.5) and np.all(tB.cpu().numpy()[:off] == -3.5)
    return Rout, V, [host(t) for t in Ts], (dR, ldr, dB, ldb, Ts)


def _gram_err(Rn, G):
    return np.linalg.norm(Rn.T @ Rn - G) / np.linalg.norm(G)


@pytest.mark.parametrize("n,p", CASES)
def test_tpqrt_gram_identity_lapack_lower_triangle_and_determinism(qr, n, p):
    n, p = _shape(qr, n, p)
    R, B = _inputs(n, p)
    plan = qr.Plan(n, n, 0, 0)
    Rout, V, Ts, _ = _tpqrt(qr, plan, R, B)
    Rn = np.triu(Rout)
    S = np.vstack([R, B])
    g = _gram_err(Rn, R.T @ R + B.T @ B)
    Rl = np.linalg.qr(S, mode="r")
    sg = np.sign(np.diag(Rl)) * np.sign(np.diag(Rn))
    kappa = np.linalg.cond(S)
    e = rel(Rn, sg[:, None] * Rl)
    print(f"tpqrt n={n} p={p}: gram {g / EPS:.2f} eps (bound {n}), R' vs LAPACK {e / EPS:.2f} eps at kappa {kappa:.1f} (bound {50 * kappa:.0f})")
    assert np.all(np.isfinite(Rout)) and np.all(np.isfinite(V))
    assert g <= n * EPS
    assert e <= 50 * kappa * EPS
    assert np.array_equal(np.tril(Rout, -1), np.tril(np.full((n, n), SENTINEL), -1)), "the strict lower triangle of dR is the caller's"
    for T in Ts:                                   # each panel's T block is upper triangular
        for k in range(0, n, TW):
            assert np.all(np.tril(T[:min(TW, n - k), k:k + TW], -1) == 0.0)
    R2, V2, T2, _ = _tpqrt(qr, plan, R, B)
    assert np.array_equal(Rout, R2) and np.array_equal(V, V2) and all(np.array_equal(a, b) for a, b in zip(Ts, T2))
    plan.close()


@pytest.mark.parametrize("n,p", CASES)
def test_tpqrt_zero_column_and_zero_start(qr, n, p):
    n, p = _shape(qr, n, p)
    R, B = _inputs(n, p)
    plan = qr.Plan(n, n, 0, 0)
    # an exactly zero column of B (R(j,j) != 0 there) gives tau = 0, an exactly zero column of V and an untouched row of R.  The column is
    # the first one: a later column of B is zero on entry only, the reflectors to its left fill it in (as in LAPACK's dtpqrt)
    j = 0
    Bz = B.copy()
    Bz[:, j] = 0.0
    assert R[j, j] != 0.0
    Rout, V, Ts, _ = _tpqrt(qr, plan, R, Bz)
    assert np.all(V[:, j] == 0.0)
    Rn = np.triu(Rout)
    assert np.array_equal(Rn[j], R[j])
    g = _gram_err(Rn, R.T @ R + Bz.T @ Bz)
    assert all(T[0, j] == 0.0 for T in Ts)         # tau_j
    # R = 0 on entry: how an accumulation starts
    R0, V0, _, _ = _tpqrt(qr, plan, np.zeros((n, n)), B)
    g0 = _gram_err(np.triu(R0), B.T @ B)
    print(f"tpqrt n={n} p={p}: zero column gram {g / EPS:.2f} eps, zero start gram {g0 / EPS:.2f} eps (bound {n})")
    assert np.all(np.isfinite(R0)) and np.all(np.isfinite(V0))
    assert g <= n * EPS and g0 <= n * EPS
    plan.close()


def test_tpqrt_keeps_an_upper_triangular_block_upper_triangular(qr):
    """exact zeros in B stay exact zeros: the block-triangular merge of the accumulator relies on it"""
    n = 96
    R, B = _inputs(n, n)
    Bt = np.triu(B)
    plan = qr.Plan(n, n, 0, 0)
    Rout, V, _, _ = _tpqrt(qr, plan, R, Bt)
    assert np.all(np.tril(V, -1) == 0.0)
    assert _gram_err(np.triu(Rout), R.T @ R + Bt.T @ Bt) <= n * EPS
    plan.close()


@pytest.mark.parametrize("n,p", [(200, 37), (600, "P")])
def test_tpmqrt_round_trip_and_norms(qr, n, p):
    n, p = _shape(qr, n, p)
    R, B = _inputs(n, p)
    plan = qr.Plan(n, n, 0, 0)
    _, _, _, (dR, ldr, dV, ldv, Ts) = _tpqrt(qr, plan, R, B)
    rng = np.random.default_rng(n + p)
    for nrhs in (1, 17, 65):
        C1, C2 = rng.random((n, nrhs)) - 0.5, rng.random((p, nrhs)) - 0.5
        ld1, ld2 = (n + 4) | 1, (p + 4) | 1
        t1, d1 = _strided(C1, ld1, 1, -3.5)
        t2, d2 = _strided(C2, ld2, 1, -3.5)
        plan.tpmqrt("T", dV, p, n, ldv, Ts[0], TW, d1, ld1, d2, ld2, nrhs)
        plan.sync()
        Y = np.vstack([_unstrided(t1, n, nrhs, ld1, 1), _unstrided(t2, p, nrhs, ld2, 1)])
        C = np.vstack([C1, C2])
        nerr = np.max(np.abs(np.linalg.norm(Y, axis=0) - np.linalg.norm(C, axis=0)) / np.linalg.norm(C, axis=0))
        plan.tpmqrt("N", dV, p, n, ldv, Ts[0], TW, d1, ld1, d2, ld2, nrhs)
        plan.sync()
        Z = np.vstack([_unstrided(t1, n, nrhs, ld1, 1), _unstrided(t2, p, nrhs, ld2, 1)])
        rerr = rel(Z, C)
        print(f"tpmqrt n={n} p={p} nrhs={nrhs}: column norms {nerr / EPS:.2f} eps, round trip {rerr / EPS:.2f} eps (bound {n + p})")
        assert rel(Y, C) > 0.1, "Q'^T is not the identity"
        assert nerr <= (n + p) * EPS and rerr <= (n + p) * EPS
        for t, rows, ld in ((t1, n, ld1), (t2, p, ld2)):       # nothing outside the blocks is written
            raw = t.cpu().numpy()
            assert raw[0] == -3.5 and np.all(raw[1:].reshape(nrhs, ld)[:, rows:] == -3.5)
    plan.close()


def test_tpmqrt_applied_to_the_stacked_matrix_gives_the_new_triangle(qr):
    n, p = 96, 7
    R, B = _inputs(n, p)
    plan = qr.Plan(n, n, 0, 0)
    Rout, _, _, (dR, ldr, dV, ldv, Ts) = _tpqrt(qr, plan, R, B)
    d1, d2 = dev(R), dev(B)
    plan.tpmqrt("T", dV, p, n, ldv, Ts[0], TW, d1, n, d2, p, n)
    plan.sync()
    out = np.vstack([host(d1), host(d2)])
    want = np.vstack([np.triu(Rout), np.zeros((p, n))])
    err = np.linalg.norm(out - want) / np.linalg.norm(np.vstack([R, B]))
    print(f"Q'^T [R ; B] - [R' ; 0]: {err / EPS:.2f} eps of |[R ; B]| (bound {n})")
    assert err <= n * EPS
    plan.close()


def test_tpqrt_refuses_more_rows_than_the_limit(qr):
    n, P = 64, _P(qr)
    plan = qr.Plan(n, n, 0, 0)
    dR, dB, dT = zeros(n, n), zeros(P + 1, n), zeros(TW, n)
    with pytest.raises(qr.QRError) as ei:
        plan.tpqrt(dR, n, n, dB, P + 1, P + 1, dT, TW)
    assert ei.value.status == qr.QR_E_ARG
    plan.close()


def _accumulate(qr, plan, acc, A, B, chunks):
    r, keep = 0, []                 # the pushes are queued on the plan's stream: the chunk buffers live until it has been drained
    for h in chunks:
        keep.append((dev(A[r:r + h]), dev(B[r:r + h])))
        acc.push(keep[-1][0], h, h, keep[-1][1], h)
        r += h
    assert r == A.shape[0]
    n, nrhs = A.shape[1], B.shape[1]
    dX, dres = zeros(n, nrhs), zeros(nrhs, 1)
    acc.solve(dX, n, dres)
    plan.sync()
    return host(dX), host(dres)[:, 0], dX, dres


@pytest.mark.parametrize("case", [1, 2])
def test_accumulator_matches_numpy(qr, case):
    P = _P(qr)
    rng = np.random.default_rng(case)
    if case == 1:
        n, chunks = 200, (1, 7, 64, 500, 513, 1915)
    else:
        n, chunks = 600, (P + 1, 599, 600, 1, 1200 - P, 599)
    m, nrhs = 3000, 3
    assert sum(chunks) == m
    A, B = rng.random((m, n)) - 0.5, rng.random((m, nrhs)) - 0.5
    plan = qr.Plan(max(max(chunks), n), n, 0, 0)
    acc = qr.LsAccumulator(plan, n, nrhs)
    X, resid, dX, dres = _accumulate(qr, plan, acc, A, B, chunks)
    assert acc.rows() == m
    kappa = np.linalg.cond(A)
    Xn = np.linalg.lstsq(A, B, rcond=None)[0]
    rn = np.linalg.norm(A @ Xn - B, axis=0)
    R, Z = acc.factor_host()
    g = _gram_err(R, A.T @ A)
    print(f"accumulator case {case}: X {rel(X, Xn) / EPS:.1f} eps at kappa {kappa:.2f}, resid {np.max(np.abs(resid - rn) / rn) / EPS:.1f} eps, "
          f"gram {g / EPS:.2f} eps (bound {n})")
    _check(A, B, X, resid, kappa)
    assert np.all(np.tril(R, -1) == 0.0)
    assert g <= n * EPS
    assert rel(np.linalg.solve(R, Z), Xn) <= 50 * kappa * kappa * EPS      # Z belongs to R
    # a second solve: the state is untouched
    acc.solve(dX, n, dres)
    plan.sync()
    assert np.array_equal(host(dX), X) and np.array_equal(host(dres)[:, 0], resid)
    # reset, the same pushes: the same bits
    acc.reset()
    assert acc.rows() == 0
    X2, resid2, _, _ = _accumulate(qr, plan, acc, A, B, chunks)
    assert np.array_equal(X2, X) and np.array_equal(resid2, resid)
    acc.close()
    plan.close()


def test_accumulator_ill_conditioned(qr):
    m, n, nrhs = 2000, 200, 2
    A = _cond_matrix(m, n, 1e8, 4)
    B = np.random.default_rng(8).random((m, nrhs)) - 0.5
    chunks = [333] * 6 + [2]
    plan = qr.Plan(333, n, 0, 0)
    acc = qr.LsAccumulator(plan, n, nrhs)
    X, resid, _, _ = _accumulate(qr, plan, acc, A, B, chunks)
    kappa = np.linalg.cond(A)
    Xn = np.linalg.lstsq(A, B, rcond=None)[0]
    rn = np.linalg.norm(A @ Xn - B, axis=0)
    bound = kappa + kappa ** 2 * np.linalg.norm(rn) / (np.linalg.norm(A, 2) * np.linalg.norm(Xn))      # the bound of _check
    print(f"accumulator cond 1e8: X {rel(X, Xn):.2e} at kappa {kappa:.2e} (bound {50 * bound * EPS:.2e}), "
          f"resid vs numpy {np.max(np.abs(resid - rn) / rn):.2e}")
    # X only: numpy's own residual A X - B carries ||A|| ||X|| eps ~ 1e-9 of rounding at |X| ~ 1e7, 1e-10 of ||r||, so it is no
    # reference for the residual norms at 1e-12 here (the well-conditioned cases check them)
    assert rel(X, Xn) <= 50 * bound * EPS
    assert np.all(np.abs(resid - rn) <= 100 * np.linalg.norm(A, 2) * np.linalg.norm(Xn, axis=0) * EPS)
    acc.close()
    plan.close()


def test_accumulator_refuses_a_tall_chunk_above_the_plan(qr):
    n = 64
    plan = qr.Plan(128, n, 0, 0)
    acc = qr.LsAccumulator(plan, n, 1)
    dA, dB = zeros(129, n), zeros(129, 1)
    with pytest.raises(qr.QRError) as ei:
        acc.push(dA, 129, 129, dB, 129)
    assert ei.value.status == qr.QR_E_ARG and acc.rows() == 0
    acc.close()
    plan.close()


def test_lstsq_chunked_matches_lstsq(qr):
    rng = np.random.default_rng(21)
    m, n, nrhs = 3000, 200, 2
    A, B = rng.random((m, n)) - 0.5, rng.random((m, nrhs)) - 0.5
    kappa = np.linalg.cond(A)
    Xl, rl = qr.lstsq(A, B)
    Xn = np.linalg.lstsq(A, B, rcond=None)[0]
    rn = np.linalg.norm(A @ Xn - B, axis=0)
    bound = kappa + kappa ** 2 * np.linalg.norm(rn) / (np.linalg.norm(A, 2) * np.linalg.norm(Xn))
    for chunk in (1000, 150, 3000):
        X, r = qr.lstsq_chunked(A, B, chunk)
        print(f"lstsq_chunked chunk {chunk}: vs lstsq {rel(X, Xl) / EPS:.1f} eps, vs numpy {rel(X, Xn) / EPS:.1f} eps (bound {50 * bound:.0f})")
        _check(A, B, X, r, kappa)
        assert rel(X, Xl) <= 50 * bound * EPS
        assert np.max(np.abs(r - rl) / rl) <= 1e-12
    x1, r1 = qr.lstsq_chunked(A, B[:, 0], 1000)
    assert x1.shape == (n,) and np.ndim(r1) == 0
    qr.release_cached_plans()


def test_lstsq_chunked_with_fewer_rows_than_columns_is_singular(qr):
    rng = np.random.default_rng(3)
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_chunked(rng.random((150, 200)), rng.random(150), 64)
    assert ei.value.status == qr.QR_E_SINGULAR
    A = rng.random((300, 40))
    A[:, 0] = 0.0                                  # a zero first column: R(0,0) == 0 exactly
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_chunked(A, np.ones(300), 100)
    assert ei.value.status == qr.QR_E_SINGULAR
