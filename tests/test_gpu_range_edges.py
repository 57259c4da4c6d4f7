"""-m gpu: range edges and small-shape accuracy of the factor, apply and substitution paths against tests/hp_ref.py.

Error measures, all evaluated in extended precision: the normwise backward error ||R x - b|| / (||R|| ||x|| + ||b||) for substitutions,
||Q_ref^T C - out|| / ||C|| for applies (Q_ref: the reflectors the kernel was given, applied in longdouble), ||A - Q R|| / ||A|| and
||Q^T Q - I|| for factorisations (Q: the factored array's reflectors formed in longdouble), the Gram residual
||R'^T R' - G|| / ||G|| for the row updates, the normal-equations residual ||A^T (A x - b)|| / (||A||^2 ||x|| + ||A|| ||b||) for
least-squares solves, the forward error against the longdouble solution for minimum-norm solves.  Each is compared with the SAME
quantity for hp_ref's float64 instance on the same input -- the same operation in working precision, never the code under test.

Bound: max(FACTOR x reference, eps), never above the bound the entry point's own test file uses (the `cap` argument of
_within: n eps for the substitutions, 3e-13 for ormqr, 1e-13 / 1e-12 for the factorisations, (n + 8) eps for the batched ones, n eps for the
Gram identity).  FACTOR is 4 (the kernels
sum in wave and tile order and the CholeskyQR routes have other constants than a Householder loop, not another order of magnitude;
the eps floor because at n = 1 the reference can be exact), except for the entries of MEASURED: cases where the kernel legitimately
exceeds 4 x, listed with the ratio measured on an MI355X in DESIGN.md ("Accuracy against the extended-precision reference"); their
bound is twice the measured ratio.  Every test prints its ratios (-s), which is how that table is regenerated.

C1 (range edge): the smallest full-rank case of every route at s = 2^480 and 2^-480 (about 1e+-144.5: inside the 1e+-150 the
suite promises elsewhere, with room for a few hundred summed squares).  Equality is not expected there (products of two small
quantities go subnormal); outputs must be finite, status words and ranks those of the unscaled run, and the error measure within the
bound of the unscaled input.
C2 (substitution and apply edges): solve_r / solve_rt at every n around the 16-row sub-step and the 64-row block, odd leading
dimensions, bases one double off, sentinel-filled buffers, every NC instantiation and both host routes; ormqr at small and ragged
shapes against the longdouble Q.
"""
import functools

import numpy as np
import pytest
import torch

import hp_ref as H
import test_gpu_batched as tb
import test_gpu_batched_pivot as tbp
import test_gpu_panel_cqr as tcq
import test_gpu_panel_fused as tpf
from gpu_util import dev, host, within, zeros
from test_gpu_downdate import _tphqrt
from test_gpu_kernels import _cholqr_leaf
from test_gpu_lstsq import _cond_matrix
from test_gpu_svd import _gesvj
from test_gpu_update import _strided, _tpqrt, _unstrided

pytestmark = pytest.mark.gpu

EPS = H.EPS
EDGE_SCALES = [1.0, 2.0 ** 480, 2.0 ** -480]
SENT = -3.5
INF = float("inf")

# (entry point, shape...) -> the ratio to the float64 reference measured on an MI355X where it exceeds 4 (DESIGN.md has the table and
# the date); the bound of such a case is twice the ratio
MEASURED = {}


def U(seed, *shape):
    return np.random.default_rng(seed).random(shape) - 0.5


def _within(tag, got, ref, cap=INF):
    """got <= min(max(FACTOR * ref, eps), cap); prints the ratio"""
    within(tag, got, ref, cap, MEASURED, _SCALE[0])


def _factor_measures(A, F, tau, jpvt=None):
    """(residual, orthogonality) of the factorisation the array (F, tau) describes, reflectors formed in extended precision"""
    n = F.shape[1]
    Ap = A if jpvt is None else A[:, jpvt]
    return H.factor_errors(Ap, H.form_q(F, tau[:n]), H.triu(F))


@functools.lru_cache(maxsize=None)
def _ref_factor(key, pivoted=False):
    """the float64 instance's measures on the (unscaled) input registered under key"""
    A = _INPUTS[key]
    if pivoted:
        F, tau, jp = H.qrp(A, np.float64)
        return _factor_measures(A, F, tau, jp)
    F, tau = H.qr(A, np.float64)
    return _factor_measures(A, F, tau)


_INPUTS = {}
_SCALE = [""]                # what _within appends to the tags it prints: the scale of the range-edge run in progress


def _input(key, make):
    if key not in _INPUTS:
        _INPUTS[key] = make()
        _INPUTS[key].setflags(write=False)
    return _INPUTS[key]


def _check_factor(tag, key, s, F, tau, jpvt=None, caps=(1e-13, 1e-12)):
    A = _INPUTS[key]
    assert np.isfinite(F).all() and np.isfinite(tau).all()
    res, orth = _factor_measures(s * A, F, tau, jpvt)
    rres, rorth = _ref_factor(key, jpvt is not None)
    _within(tag + " resid", res, rres, caps[0])
    _within(tag + " orth", orth, rorth, caps[1])


# =====================================================================================================================================
# C2: substitution and apply edges
# =====================================================================================================================================
TRSM_N = [1, 15, 16, 17, 63, 64, 65, 127, 129, 200]
TRSM_NRHS = [1, 2, 4, 5, 16, 17, 64, 65]


@functools.lru_cache(maxsize=None)
def _triangle(qr, kind, n):
    """the factored n x n array of Plan.geqrf on a uniform (kind 'uniform') or a cond-1e10 matrix, as numpy; read-only"""
    A = U(n, n, n) if kind == "uniform" else _cond_matrix(n, n, 1e10, n)
    p = qr.Plan(n, n, 0, 0)
    dA, dtau = dev(A), zeros(n, 1)
    p.geqrf(dA, n, n, n, dtau)
    p.sync()
    F = host(dA)
    p.close()
    assert np.isfinite(F).all() and np.all(np.diag(F) != 0.0)
    F.setflags(write=False)
    return F


@pytest.mark.parametrize("n", TRSM_N)
@pytest.mark.parametrize("kind", ["uniform", "cond1e10"])
@pytest.mark.parametrize("which", ["solve_r", "solve_rt"])
def test_substitution_edges(qr, which, kind, n):
    F = _triangle(qr, kind, n)
    trans = which == "solve_rt"
    Ball = U(1000 + n, n, max(TRSM_NRHS))
    ref = (H.solve_rt if trans else H.solve_r)(H.triu(F), Ball, np.float64)
    ref_err = H.trsm_backward_errors(F, ref, Ball, trans)
    lda, ldb, off = n + 3, n + 5, 1
    p = qr.Plan(n, n, 0, 0)
    tA, dA = _strided(F, lda, off, SENT)
    a0 = tA.cpu().numpy().copy()
    for nrhs in TRSM_NRHS:
        Bm = Ball[:, :nrhs]
        tB, dB = _strided(Bm, ldb, off, SENT)
        getattr(p, which)(dA, n, lda, dB, nrhs, ldb)
        p.sync()
        raw = tB.cpu().numpy()
        assert np.all(raw[:off] == SENT) and np.all(raw[off:].reshape(nrhs, ldb)[:, n:] == SENT), "written outside the n x nrhs block"
        X = _unstrided(tB, n, nrhs, ldb, off)
        assert np.isfinite(X).all()
        err = H.trsm_backward_errors(F, X, Bm, trans).max()
        _within(f"{which} {kind} n={n} nrhs={nrhs}", err, ref_err[:nrhs].max(), n * EPS)
    assert np.array_equal(tA.cpu().numpy(), a0), "the triangle's array is read only"
    p.close()


@pytest.mark.parametrize("m,n", [(1, 1), (17, 16), (65, 63), (64, 64), (600, 33), (1100, 37)])
def test_ormqr_edges(qr, m, n):
    A = U(m * 7 + n, m, n)
    p = qr.Plan(m, n, 0, 0)
    nb = p.nb
    dA, dtau = dev(A), zeros(n, 1)
    p.geqrf(dA, m, n, m, dtau)
    dT = zeros(nb, n)
    p.build_t(dA, m, n, m, dtau, dT, nb)
    p.sync()
    F, tau = host(dA), host(dtau)[:, 0]
    ldc, off = m + 5, 1
    for nrhs in (1, 4, 5, 17):
        Cm = U(nrhs + m, m, nrhs)
        for trans in "TN":
            want = H.apply_q(F, tau, Cm, trans)
            ref_err = H.apply_error(want, H.apply_q(F, tau, Cm, trans, np.float64), Cm)
            for T, ldt in ((None, 0), (dT, nb)):
                tC, dC = _strided(Cm, ldc, off, SENT)
                p.ormqr(trans, dA, m, n, m, dtau, dC, nrhs, ldc, dT=T, ldt=ldt)
                p.sync()
                raw = tC.cpu().numpy()
                assert np.all(raw[:off] == SENT) and np.all(raw[off:].reshape(nrhs, ldc)[:, m:] == SENT), "written outside the m x nrhs block"
                out = _unstrided(tC, m, nrhs, ldc, off)
                _within(f"ormqr {trans} {m}x{n} nrhs={nrhs} T={'given' if T is not None else 'rebuilt'}", H.apply_error(want, out, Cm), ref_err,
                        3e-13)
    assert np.array_equal(host(dA), F), "the factors are read only"
    p.close()


# =====================================================================================================================================
# C1: the range edge, one smallest full-rank case per route
# =====================================================================================================================================
@pytest.fixture(scope="module")
def q(qr):
    tcq.q.__wrapped__(qr)
    tpf.q.__wrapped__(qr)
    return qr


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)
    yield p
    p.close()


_STATUS = {}


def _same_status(key, s, value):
    """status words, ranks and counters must be those of the unscaled run (which comes first in EDGE_SCALES)"""
    value = np.asarray(value)
    if s == 1.0:
        _STATUS[key] = value
    assert key in _STATUS and np.array_equal(_STATUS[key], value), (key, s, _STATUS.get(key), value)


def _edge_guarded_leaf_panel(qr, plan, s):
    """513 rows (odd: straight to the Householder TSQR) and 514 (the CholeskyQR2 route, which must accept at every scale)"""
    for mk in (513, 514):
        P = _input(("leaf", mk), lambda: U(mk, mk, 32))
        out, tau, T, V, guard, _ = _cholqr_leaf(qr, s * P)
        _same_status(("leaf", mk), s, guard)
        assert guard == 0 and np.isfinite(T).all() and np.isfinite(V).all()
        _check_factor(f"leaf panel {mk}x32", ("leaf", mk), s, out, tau)


def _edge_one_launch_panel(qr, plan, s):
    P = _input("fused", lambda: U(288, 256, 32))
    out, V, T, tau, G, st = tpf.run_panel(qr, tpf.Ws(qr), s * P)
    _same_status("fused", s, st)
    assert st[0] == 0 and st[1] == 0 and np.isfinite(V).all()
    _check_factor("one-launch panel 256x32", "fused", s, out, tau)


def _edge_full_width_panel(qr, plan, s):
    P = _input("cqr", lambda: U(428, 300, 128))
    out, V, T, tau, st = tcq.run_panel(qr, s * P, qbuf=True)
    _same_status("cqr", s, st[:1])
    assert st[0] == 0 and np.isfinite(V).all() and np.isfinite(T).all()
    _check_factor("full-width panel 300x128", "cqr", s, out, tau)


def _edge_geqrf(qr, plan, s):
    m, n = 65, 63
    A = _input("geqrf", lambda: U(m * n, m, n))
    p = qr.Plan(m, n, 0, 0)
    dA, dtau = dev(s * A), zeros(n, 1)
    p.geqrf(dA, m, n, m, dtau)
    p.sync()
    stats = p.route_stats()
    p.close()
    _same_status("geqrf", s, [stats[k] for k in sorted(stats)])
    _check_factor("geqrf 65x63", "geqrf", s, host(dA), host(dtau)[:, 0])


def _edge_mmqr_and_explicit_qr(qr, plan, s):
    A = _input("mmqr", lambda: U(4, 200, 40))
    F, tau = qr.mmqr(s * A)
    Q, R = qr.explicit_qr(F, tau)
    assert np.isfinite(F).all() and np.isfinite(tau).all() and np.isfinite(Q).all() and np.isfinite(R).all()
    res, orth = H.factor_errors(s * A, Q[:, :40], R[:40])
    rres, rorth = _ref_factor("mmqr")
    _within("mmqr + explicitQR 200x40 resid", res, rres, 1e-13)
    _within("mmqr + explicitQR 200x40 orth", orth, rorth, 1e-12)


def _edge_section3_ormqr_solve_r_gels(qr, plan, s):
    m, n, nrhs = 1000, 37, 3
    A = _input("gels", lambda: U(1037, m, n))
    B = U(1038, m, nrhs)
    p = qr.Plan(m, n, 0, 0)
    dA, dtau, dB = dev(s * A), zeros(n, 1), dev(B)
    p.gels(dA, m, n, m, dtau, dB, nrhs, m)
    p.sync()
    F, tau, X = host(dA), host(dtau)[:, 0], host(dB)[:n]
    assert np.isfinite(X).all()
    _check_factor("gels 1000x37 factors", "gels", s, F, tau)
    Xr, _ = H.lstsq(A, B, np.float64)
    _within("gels 1000x37 normal equations", H.normal_equations_residual(s * A, X, B), H.normal_equations_residual(A, Xr, B))
    # the apply and the substitution on their own, from these factors
    Cm = U(1039, m, 4)
    dC = dev(Cm)
    p.ormqr("T", dA, m, n, m, dtau, dC, 4, m)
    p.sync()
    want = H.apply_q(F, tau, Cm, "T")
    _within("ormqr T 1000x37 nrhs=4 (edge)", H.apply_error(want, host(dC), Cm), H.apply_error(want, H.apply_q(F, tau, Cm, "T", np.float64), Cm), 3e-13)
    Y = U(1040, n, nrhs)
    dY = dev(Y)
    p.solve_r(dA, n, m, dY, nrhs, n)
    p.sync()
    R = H.triu(F)
    _within("solve_r n=37 (edge)", H.trsm_backward_error(R, host(dY), Y), H.trsm_backward_error(R, H.solve_r(R, Y, np.float64), Y), n * EPS)
    p.close()


def _edge_section4_geqp3_rank_gelsp(qr, plan, s):
    m, n, nrhs = 300, 70, 3
    A = _input("geqp3", lambda: U(370, m, n))
    B = U(372, m, nrhs)
    p = qr.Plan(m, n, 0, 0)
    dA, dtau, dj = dev(s * A), zeros(n, 1), torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p.geqp3(dA, m, n, m, dj, dtau)
    r = p.rank(dA, m, n, m)
    p.sync()
    jp = dj.cpu().numpy().astype(np.int64)
    assert sorted(jp) == list(range(n))
    _check_factor("geqp3 300x70", "geqp3", s, host(dA), host(dtau)[:, 0], jp)
    dA2, dB, dres = dev(s * A), dev(B), zeros(nrhs, 1)
    r2 = p.gelsp(dA2, m, n, m, dj, dtau, dB, nrhs, m, dresid=dres)
    p.sync()
    p.close()
    _same_status("geqp3 ranks", s, [r, r2])
    assert r == n and r2 == n and np.isfinite(host(dres)).all()
    Xr, _ = H.lstsq(A, B, np.float64)
    _within("gelsp 300x70 normal equations", H.normal_equations_residual(s * A, host(dB)[:n], B), H.normal_equations_residual(A, Xr, B))


def _edge_section5_solve_rt_gels_wide(qr, plan, s):
    m, n, nrhs = 300, 70, 3                         # the tall shape: the wide system is n x m
    A = _input("wide", lambda: U(5300, m, n))
    B = U(5301, n, nrhs)
    p = qr.Plan(m, n, 0, 0)
    Bp = np.zeros((m, nrhs))
    Bp[:n] = B
    dW, dF, dtau, dB = dev(s * A.T), zeros(m, n), zeros(n, 1), dev(Bp)
    p.gels_wide(dW, n, m, n, dF, m, dtau, dB, nrhs, m)
    p.sync()
    F, tau, X = host(dF), host(dtau)[:, 0], host(dB)
    assert np.isfinite(X).all()
    _check_factor("gels_wide 70x300 factors", "wide", s, F, tau)
    Xl = H.minnorm(A.T, B)                              # longdouble, unscaled: the scaled system's solution is exactly Xl / s
    fwd = lambda Z: float(H.norm(H.arr(Z) - Xl) / H.norm(Xl))
    _within("gels_wide 70x300 forward error", fwd(H.arr(X) * H.arr(s)), fwd(H.minnorm(A.T, B, np.float64)))
    Y = U(5302, n, nrhs)
    dY = dev(Y)
    p.solve_rt(dF, n, m, dY, nrhs, n)
    p.sync()
    R = H.triu(F)
    _within("solve_rt n=70 (edge)", H.trsm_backward_error(R, host(dY), Y, True), H.trsm_backward_error(R, H.solve_rt(R, Y, np.float64), Y, True),
            n * EPS)
    p.close()


def _gram_error(Rn, G):
    Rn = H.arr(H.triu(Rn))
    return float(H.norm(H.matmul(Rn.T, Rn) - G) / H.norm(G))


def _edge_section6_row_updates_and_accumulator(qr, plan, s):
    n, p_add, p_del, nrhs = 33, 4, 3, 2
    X = _input("update", lambda: U(633, 2 * n + 7, n))
    R = np.triu(np.linalg.qr(X, mode="r"))
    Bnew = U(634, 7, n)
    plan = qr.Plan(2 * n + 7, n, 0, 0)
    # append 7 rows
    Rout, V, Ts, _ = _tpqrt(qr, plan, s * R, s * Bnew)
    assert np.isfinite(Rout[np.triu_indices(n)]).all() and np.isfinite(V).all() and np.isfinite(Ts[0]).all()
    G = H.matmul(H.arr(R).T, H.arr(R)) + H.matmul(H.arr(Bnew).T, H.arr(Bnew))
    ref = _gram_error(H.append_rows(R, Bnew, np.float64)[0], G)
    _within("tpqrt n=33 p=7 gram", _gram_error(np.triu(Rout) / s, G), ref, n * EPS)
    # add 4 rows and remove the last 3 rows of X in one pass
    Bm = np.vstack([Bnew[:p_add], X[-p_del:]])
    Rout, V, T, _ = _tphqrt(qr, plan, s * R, s * Bm, p_add, p_del)
    assert np.isfinite(Rout[np.triu_indices(n)]).all() and np.isfinite(V).all() and np.isfinite(T).all()
    G = H.matmul(H.arr(R).T, H.arr(R)) + H.matmul(H.arr(Bm[:p_add]).T, H.arr(Bm[:p_add])) - H.matmul(H.arr(X[-p_del:]).T, H.arr(X[-p_del:]))
    ref = _gram_error(H.remove_rows(np.vstack([X, Bm[:p_add]]), np.r_[0:2 * n + 7 - p_del, 2 * n + 7:2 * n + 7 + p_add], np.float64), G)
    _within("tphqrt n=33 +4 -3 gram", _gram_error(np.triu(Rout) / s, G), ref, n * EPS)
    # the accumulator: push all rows, pop 7, solve
    Bv = U(635, 2 * n + 7, nrhs)
    acc = qr.LsAccumulator(plan, n, nrhs)
    d1, d2, d3, d4 = dev(s * X), dev(Bv), dev(s * X[10:17]), dev(Bv[10:17])
    acc.push(d1, 2 * n + 7, 2 * n + 7, d2, 2 * n + 7)
    plan.sync()
    acc.pop(d3, 7, 7, d4, 7)
    dX = zeros(n, nrhs)
    acc.solve(dX, n)
    plan.sync()
    _same_status("lsacc rows", s, acc.rows())
    acc.close()
    plan.close()
    keep = np.r_[0:10, 17:2 * n + 7]
    Xr, _ = H.lstsq(X[keep], Bv[keep], np.float64)
    _within("lsacc push pop solve n=33 normal equations", H.normal_equations_residual(s * X[keep], host(dX), Bv[keep]),
            H.normal_equations_residual(X[keep], Xr, Bv[keep]))


def _edge_section7_gesvj(qr, plan, s):
    """no float64 instance of a Jacobi SVD exists in hp_ref: the bound is the one tests/test_gpu_svd.py derives for this kernel,
    sweeps x n x eps, for the reconstruction and both orthogonalities (one rotation per pair and sweep, each an eps-sized perturbation)"""
    n = 33
    G = _input("gesvj", lambda: U(733, n, n))
    plan = qr.Plan(n, n, 0, 0)
    Uv, S, V, sw = _gesvj(plan, s * G)
    plan.close()
    _same_status("gesvj sweeps", s, sw)
    assert np.isfinite(Uv).all() and np.isfinite(S).all() and np.isfinite(V).all() and np.all(S[:-1] >= S[1:]) and S[-1] > 0
    Ul, Vl = H.arr(Uv), H.arr(V)
    rec = float(H.norm(H.matmul(Ul * H.arr(S / s)[None, :], Vl.T) - H.arr(G)) / H.norm(G))
    ou = float(H.norm(H.matmul(Ul.T, Ul) - H.arr(np.eye(n))))
    ov = float(H.norm(H.matmul(Vl.T, Vl) - H.arr(np.eye(n))))
    bound = sw * n * EPS
    print(f"RATIO gesvj 33x33 at 2^{np.log2(s):.0f}: reconstruction {rec / EPS:.1f} eps, U {ou / EPS:.1f} eps, V {ov / EPS:.1f} eps; bound {sw * n} eps")
    assert rec <= bound and ou <= bound and ov <= bound


def _edge_section8_batched(qr, plan, s):
    """17 x 17 (the wave route) and 100 x 33 (the workgroup route of the unpivoted and of the bp_* kernels)"""
    for m, n in ((17, 17), (100, 33)):
        key = "batched" if m == 17 else ("batched", m, n)
        A = _input(key, lambda: U(8117 + (m != 17) * (m + n), 3, m, n))
        Bm = U(8118 + (m != 17) * (m + n), 3, m, 2)
        F, tau, _ = tb._factor(plan, s * A, with_q=False)
        X, rss, info = tb._gels(plan, s * A, Bm)
        Fp, taup, jp, _ = tbp._geqp3(plan, s * A, with_q=False)
        Xy, resid, rank, jp2, _, _, _ = tbp._solve(plan, s * A, Bm, True)
        _same_status(key, s, np.concatenate([info, rank, jp.ravel(), jp2.ravel()]))
        assert not info.any() and np.all(rank == n) and np.isfinite(X).all() and np.isfinite(Xy).all() and np.isfinite(resid).all()
        assert np.isfinite(rss).all()
        for k in range(3):
            ck = ("batched", k) if m == 17 else ("batched", m, n, k)
            _input(ck, lambda: A[k].copy())
            _check_factor(f"geqrf_batched {m}x{n} [{k}]", ck, s, F[k], tau[k], caps=((n + 8) * EPS, (n + 8) * EPS))
            _check_factor(f"geqp3_batched {m}x{n} [{k}]", ck, s, Fp[k], taup[k], jp[k], caps=((n + 8) * EPS, (n + 8) * EPS))
            Xr, _ = H.lstsq(A[k], Bm[k], np.float64)
            rne = H.normal_equations_residual(A[k], Xr, Bm[k])
            _within(f"gels_batched {m}x{n} [{k}] normal equations", H.normal_equations_residual(s * A[k], X[k], Bm[k]), rne)
            _within(f"gelsy_batched {m}x{n} [{k}] normal equations", H.normal_equations_residual(s * A[k], Xy[k], Bm[k]), rne)


EDGE_CASES = {f.__name__[6:]: f for f in (_edge_guarded_leaf_panel, _edge_one_launch_panel, _edge_full_width_panel, _edge_geqrf,
                                          _edge_mmqr_and_explicit_qr, _edge_section3_ormqr_solve_r_gels, _edge_section4_geqp3_rank_gelsp,
                                          _edge_section5_solve_rt_gels_wide, _edge_section6_row_updates_and_accumulator,
                                          _edge_section7_gesvj, _edge_section8_batched)}


@pytest.mark.parametrize("case", list(EDGE_CASES))
def test_range_edge(q, plan, case):
    """the case unscaled, then at 2^480 and 2^-480"""
    try:
        for s in EDGE_SCALES:
            _SCALE[0] = f" @2^{int(np.log2(s))}"
            EDGE_CASES[case](q, plan, s)
    finally:
        _SCALE[0] = ""
