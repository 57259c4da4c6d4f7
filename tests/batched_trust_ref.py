"""A numpy restatement of the batched trust-region step (mi355x_qr.h section 8g; kernels: csrc/qr_batched_trust.hip) for one member, with
the inputs and the truth of its tests (helper module, no fixtures, no GPU).

lmpar() is MINPACK lmpar (More 1978) with par = lambda^2, parameterised by dtype like hp_ref.py: the Gauss-Newton step over the leading
nsing x nsing block, the bounds parl and paru, then Newton steps on par.  Every elimination is batched_damped_ref.solve (the solution,
|D x| and the residual of lambda = sqrt(par)) and batched_damped_ref.step (the damped triangle the correction needs).

The truth of a result (lambda, x): |D x(lambda)| in longdouble from hp_ref.lstsq on the stacked system [A ; lambda D] x = [b ; 0]
(batched_damped_ref.truth).

Inputs as in the damped tests: entries uniform in (-0.5, 0.5), d uniform in [0.5, 2]; every third member has its singular values graded
to condition 1e6.  Delta = f x the Gauss-Newton |D x|, f cycling over FRACS by member: f >= 1.05 accepts the Gauss-Newton step (status 1),
the others take from one to several iterations, so neighbouring members run different numbers of them.
"""
import numpy as np

import batched_damped_ref as D
import hp_ref as H

LD = H.LD
EPS = H.EPS
FRACS = (2.0, 1.05, 0.5, 1e-2, 1e-6)
RTOLS = (0.1, 1e-3)
MAXIT = 10
# the orders of the triangle: every wave width, both edges of the wave route (n + 1 = 32, 33), the LDS limit of the workgroup route
ORDERS = (1, 3, 15, 17, 31, 32, 33, 63)
TINY = float(np.finfo(np.float64).tiny)


def member(seed, m, n, graded=False):
    """A (m x n), b (m), d (n); graded: the min(m, n) singular values of A log-spaced from 1 to 1e-6"""
    A = D.U(seed, m, n)
    if graded and min(m, n) > 1:
        u, _, vt = np.linalg.svd(A, full_matrices=False)
        A = (u * np.logspace(0, -6, min(m, n))) @ vt
    b = D.U(seed + 500000, m)
    d = 0.5 + 1.5 * np.random.default_rng(seed + 900000).random(n)
    return A, b, d


def batch(m, n, count, salt=0, with_d=True):
    """`count` seeded members, every third one graded: A (count, m, n), b (count, m), d (count, n) or None"""
    ms = [member(1000 * m + 10 * n + q + 77777 * salt, m, n, q % 3 == 2) for q in range(count)]
    A, b, d = (np.stack(x) for x in zip(*ms))
    return A, b, (d if with_d else None)


def factors(A, b):
    """float64 factors of a tall member: R (n x n), z = the top of Q^T b, rss = the tail sum of squares"""
    m, n = A.shape
    Q, R = np.linalg.qr(A, mode="complete")
    y = Q.T @ b
    return np.triu(R[:n]), y[:n].copy(), float((y[n:] * y[n:]).sum())


def gauss_newton_dxnorm(R, z, d=None, jpvt=None):
    """|D x| of the Gauss-Newton step from full-rank factors, in float64: the scale the radii of the tests are fractions of"""
    n = R.shape[0]
    jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
    dd = np.ones(n) if d is None else np.asarray(d)[jp]
    return float(np.linalg.norm(dd * np.linalg.solve(np.triu(R), z)))


G_WINDOW = 256


def gradient_norm(g, dtype=np.float64):
    """|g| as bt_wave_gnorm of qr_batched_trust_dev.h forms it: the plain sum of squares while the largest |g_j| lies within
    2^-+G_WINDOW (or is 0, or no finite number); outside it g is first scaled by the power of two that brings that entry into [1, 2)"""
    g = H.arr(g, dtype)
    gmax = abs(g).max() if g.size else 0.0
    lo, hi = np.ldexp(1.0, -G_WINDOW), np.ldexp(1.0, G_WINDOW)
    if gmax == 0 or lo <= gmax <= hi or not np.isfinite(float(gmax)):
        return H._root((g * g).sum(), dtype)
    e = int(np.frexp(gmax)[1]) - 1
    gs = np.ldexp(g, -e)
    return np.ldexp(H._root((gs * gs).sum(), dtype), e)


def lmpar(R, z, delta, d=None, jpvt=None, rss=None, flip=False, lam0=0.0, rtol=0.1, maxit=MAXIT, dtype=np.float64):
    """one member from factors: dict(X, lam, xnorm, resid, iter, status, info).  info != 0: the rest is None"""
    fail = lambda info: dict(X=None, lam=None, xnorm=None, resid=None, iter=None, status=None, info=info)
    if not (np.isfinite(delta) and delta > 0):
        return fail(-1)
    R0, z0 = H.arr(np.triu(np.asarray(R)), dtype), H.arr(z, dtype)
    n = R0.shape[0]
    if flip:
        assert d is None and jpvt is None
        R0, z0 = R0.T[::-1, ::-1].copy(), z0[::-1].copy()
    jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
    dd = H.arr(np.ones(n) if d is None else np.asarray(d)[jp], dtype)       # d in pivoted order: the eliminations below take no jpvt
    tail = None if rss is None else [rss]
    delta, rtol = H.arr(delta, dtype), H.arr(rtol, dtype)
    nrm = lambda v: H._root((v * v).sum(), dtype)

    def finish(x, lam, xnorm, it, status):
        E = -z0.copy()
        E = (R0 * x[None, :]).sum(axis=1) + E
        resid = H._root((E * E).sum() + H.arr(0.0 if rss is None else rss, dtype), dtype)
        X = x * 0
        X[(n - 1 - np.arange(n)) if flip else jp] = x
        return dict(X=X, lam=lam, xnorm=xnorm, resid=resid, iter=it, status=status, info=0)

    nsing = n
    for i in range(n):
        if R0[i, i] == 0:
            nsing = i
            break
    x = z0 * 0
    if nsing:
        x[:nsing] = H.solve_r(R0[:nsing, :nsing], z0[:nsing], dtype)
    dxnorm = nrm(dd * x)
    fp = dxnorm - delta
    if fp <= rtol * delta:
        return finish(x, H.arr(0.0, dtype), dxnorm, 0, 1)
    parl = H.arr(0.0, dtype)
    if nsing == n:
        w = nrm(H.solve_rt(R0, dd * ((dd * x) / dxnorm), dtype))
        parl = ((fp / delta) / w) / w
    g = np.array([(R0[:j + 1, j] * z0[:j + 1]).sum() / dd[j] if dd[j] != 0 else 0 * dd[j] for j in range(n)])
    gnorm = gradient_norm(g, dtype)
    paru = gnorm / delta
    if paru == 0:
        paru = H.arr(TINY, dtype) / min(delta, H.arr(0.1, dtype))
    par = min(max(H.arr(lam0, dtype) ** 2, parl), paru)
    if par == 0:
        par = gnorm / dxnorm
    it = 0
    while True:
        it += 1
        if par == 0:
            par = max(H.arr(TINY, dtype), H.arr(0.001, dtype) * paru)
        lam = H._root(par, dtype)
        X, xn, _, info = D.solve(R0, z0[:, None], lam, dd, None, tail, False, dtype)
        if info:
            return fail(info)
        x, dxnorm = X[:, 0], xn[0]
        prev, fp = fp, dxnorm - delta
        if abs(fp) <= rtol * delta:
            return finish(x, lam, dxnorm, it, 0)
        if parl == 0 and fp <= prev and prev < 0:
            return finish(x, lam, dxnorm, it, 2)
        if it >= maxit:
            return finish(x, lam, dxnorm, it, 3)
        Rt, _ = D.step(R0, z0[:, None], lam * dd, dtype)
        w = nrm(H.solve_rt(Rt, dd * ((dd * x) / dxnorm), dtype))
        parc = ((fp / delta) / w) / w
        if fp > 0:
            parl = max(parl, par)
        if fp < 0:
            paru = min(paru, par)
        par = max(parl, par + parc)


def meets_rule(xnorm, lam, delta, rtol):
    """the termination rule on the numbers a call returns, in the expressions the search decides on: fp = |D x| - Delta against
    rtol Delta (fp <= rtol Delta is |D x| <= (1 + rtol) Delta)"""
    fp = xnorm - delta
    return fp <= rtol * delta if lam == 0 else abs(fp) <= rtol * delta


def norm_slack(n):
    """the relative rounding of |D x| itself: n products, a sum of n squares, a root"""
    return (n + 4) * EPS
