"""Inputs, the restatement and the error measures of the batched covariance, standard error and leverage tests (mi355x_qr.h section 8k;
helper module, no fixtures, no GPU).

The restatement follows the header's steps in straight numpy loops, parametrised by dtype: the weighted image (row i of [A | b] times
sqrt(p_i), excluded rows zero), Householder QR with b riding along (hp_ref.qr), the back substitution (hp_ref.solve_r), the triangle
inverse along the rows (T R = I), S = T T^T, the forward substitution with R^T for the leverages, and the pivoted / rank-deficient
scatter.  Its float64 instance is "the same operation in working precision" that the GPU test compares the kernels' errors with; its
longdouble instance is the reference.

A case is (m, n, weighted): `BATCH` members from numpy's default_rng(seed(m, n))
    A        standard normal m x n; every third member (q % 3 == 1) has its columns graded to 1e4
    b        A x* + 0.01 noise, x* standard normal (scaled inversely to the grading)
    p        weighted: uniform in [0.25, 4], and a quarter of the spare rows ((m - n) // 4) masked with p = 0; else None

Measures per member against the longdouble instance, kappa the 2-norm condition of diag(sqrt(p)) A (its included rows):
    C    ||C - C_ref||_F / ||C_ref||_F          se   max |se - se_ref| / max se_ref          h   max |h - h_ref|
each capped at 50 kappa eps.
"""
import functools

import numpy as np

import batched_irls_ref as IR
import hp_ref as H

EPS = H.EPS
BATCH = 9
CAP = 50.0
NAMES = ("C", "se", "h")
INF = np.inf

# (m, n) of the fused call: both routes and their edges (wave: m <= 64 and n + 1 <= 32)
FIT_SHAPES = [(1, 1), (2, 1), (5, 3), (16, 8), (33, 7), (64, 31), (64, 32), (65, 15), (100, 33), (256, 63), (300, 40), (512, 31)]
# n of the from-factor calls: the wave route up to 32, the workgroup route above
FACTOR_N = [1, 2, 7, 31, 32, 33, 63, 64]


def seed(m, n):
    return 8110000 + 1000 * m + n


def max_rows(n):
    """qr_stats_batched_max_rows from its byte formula: the largest m <= 512 with 8 ((n + 1) ld(m) + n + 72) <= 160 KiB, ld(m) the
    smallest value >= m that is 2 mod 32"""
    if n < 1 or n > 63:
        return 0
    m = 512
    while m >= n and 8 * ((n + 1) * (((m + 29) // 32) * 32 + 2) + n + 72) > 160 * 1024:
        m -= 1
    return m if m >= n else 0


def fit_wave_route(m, n):
    return m <= 64 and n + 1 <= 32


@functools.lru_cache(maxsize=None)
def make_case(m, n, weighted, batch=BATCH):
    """(A (batch, m, n), b (batch, m), p (batch, m) or None), float64, read-only"""
    rng = np.random.default_rng(seed(m, n))
    A = rng.standard_normal((batch, m, n))
    xs = rng.standard_normal((batch, n))
    grade = np.logspace(0.0, 4.0, n) if n > 1 else np.ones(1)
    for q in range(batch):
        if q % 3 == 1:
            A[q] *= grade[None, :]
            xs[q] /= grade
    b = np.einsum("qij,qj->qi", A, xs) + 0.01 * rng.standard_normal((batch, m))
    p = None
    if weighted:
        p = rng.uniform(0.25, 4.0, (batch, m))
        k = (m - n) // 4
        for q in range(batch):
            if k:
                p[q, rng.choice(m, k, replace=False)] = 0.0
        p.setflags(write=False)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b, p


def kappa(A, p=None):
    """the 2-norm condition of diag(sqrt(p)) A"""
    W = np.asarray(A, dtype=np.float64)
    if p is not None:
        W = W * np.sqrt(np.asarray(p, dtype=np.float64))[:, None]
    s = np.linalg.svd(W, compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else INF


def tri_inverse(R, r=None, dtype=np.float64):
    """T = R11^-1 (r x r) along the rows: s = (i == j), s -= T(i,k) R(k,j) for k ascending, T(i,j) = s / R(j,j); zeros left of the diagonal"""
    R = H.arr(R, dtype)
    r = R.shape[0] if r is None else r
    T = H.arr(np.zeros((r, r)), dtype)
    one = H.arr(np.ones(1), dtype)[0]
    for j in range(r):
        s = H.arr(np.zeros(r), dtype)
        s[j] = one
        for k in range(j):
            s = s - T[:, k] * R[k, j]
        col = s / R[j, j]
        col[j + 1:] = col[j + 1:] * 0
        T[:, j] = col
    return T


def covar_from_r(R, jpvt=None, rank=None, mult=1.0, dtype=np.float64):
    """(C, se) of MINPACK's covar: C = mult P [(R11^T R11)^-1 0; 0 0] P^T through T = R11^-1 and T T^T (k ascending), both triangles from
    the one value, exact zeros at the dropped variables; se = sqrt(diag C)"""
    R = H.arr(R, dtype)
    n = R.shape[0]
    r = n if rank is None else int(rank)
    jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
    T = tri_inverse(R[:r, :r], r, dtype)
    C = H.arr(np.zeros((n, n)), dtype)
    mult = H.arr(np.float64(mult), dtype)
    for j in range(r):
        s = T[:j + 1, j] * 0
        for k in range(j, r):
            s = s + T[:j + 1, k] * T[j, k]
        c = mult * s
        C[jp[:j + 1], jp[j]] = c
        C[jp[j], jp[:j + 1]] = c
    se = H._root(np.diagonal(C).copy(), dtype)
    return C, se


def leverage_from_r(R, rows, prior=None, jpvt=None, rank=None, dtype=np.float64):
    """h_i = p_i |R11^-T (P^T a_i)(0 : r)|^2 by forward substitution with R^T (ascending), the squares added in ascending order; exactly 0
    where p_i == 0 (such a row is not used)"""
    R = H.arr(R, dtype)
    n = R.shape[0]
    r = n if rank is None else int(rank)
    jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
    rows = np.asarray(rows, dtype=np.float64)
    mrows = rows.shape[0]
    p64 = np.ones(mrows) if prior is None else np.asarray(prior, dtype=np.float64)
    incl = p64 > 0
    Y = H.arr(np.where(incl[:, None], rows[:, jp[:r]], 0.0), dtype)       # mrows x r
    ss = H.arr(np.zeros(mrows), dtype)
    for k in range(r):
        s = Y[:, k]
        for l in range(k):
            s = s - R[l, k] * Y[:, l]
        Y[:, k] = s / R[k, k]
        ss = ss + Y[:, k] * Y[:, k]
    h = H.arr(p64, dtype) * ss
    h[~incl] = h[~incl] * 0
    return h


def fit_stats(A, b, prior=None, scaled=True, dtype=np.float64):
    """dict(x, e, h, sigma2, dof, C, se, info) of qr_gels_stats_batched_dev for one member in `dtype`; everything but info is None where
    the call writes nothing"""
    m, n = np.shape(A)
    nothing = dict(x=None, e=None, h=None, sigma2=None, dof=None, C=None, se=None)
    p64 = np.ones(m) if prior is None else np.asarray(prior, dtype=np.float64)
    if any(not (v >= 0 and v < INF) for v in p64):
        return dict(nothing, info=-1)
    incl = p64 > 0
    cnt = int(incl.sum())
    dof = cnt - n
    if cnt < n:
        return dict(nothing, info=-2)
    if scaled and dof == 0:
        return dict(nothing, info=-3)
    A0 = H.arr(np.where(incl[:, None], A, 0.0), dtype)                    # an excluded row is zeros whatever it holds
    b0 = H.arr(np.where(incl, b, 0.0), dtype)
    p = H.arr(p64, dtype)
    sq = H._root(p, dtype)
    F, _ = H.qr(np.column_stack([A0 * sq[:, None], b0 * sq]), dtype)      # b rides along
    R = H.triu(F[:n, :n])
    for i in range(n):
        if R[i, i] == 0:
            return dict(nothing, info=i + 1)
    x = H.solve_r(R, F[:n, n], dtype)
    e = IR.residual(np.asarray(A0, dtype=np.float64), np.asarray(b0, dtype=np.float64), x) if dtype is np.float64 else b0 - A0 @ x
    e[~incl] = e[~incl] * 0
    ssum = ((p * e) * e).sum()
    sigma2 = ssum / dof if dof > 0 else H.arr(np.float64(INF), dtype)
    h = leverage_from_r(R, A, prior, dtype=dtype)
    C, se = covar_from_r(R, dtype=dtype)
    res = dict(x=x, e=e, h=h, sigma2=sigma2, dof=dof, C=C, se=se, info=0)
    return with_scale(res, dtype) if scaled else res


def with_scale(res, dtype=np.float64):
    """the result of the scaled call from that of the unscaled one: C times sigma2 (one rounded product per entry), se = sqrt(diag C)"""
    C = res["C"] * res["sigma2"]
    return dict(res, C=C, se=H._root(np.diagonal(C).copy(), dtype))


def scaled_reference(ref, sigma2):
    """what the scaled call must return given the multiplier `sigma2` it used: C = sigma2 C_ref in the reference precision.  The relative
    error of sigma2 itself is NOT of order kappa eps (the residuals are small against b, so theirs is about eps ||b|| / ||e||); it has
    its own bound (residual_scales), and the product rule C_scaled = sigma2 C_unscaled is asserted bitwise"""
    return with_scale(dict(ref, sigma2=H.arr(np.float64(sigma2))), H.LD)


def residual_scales(A, b, p, ref):
    """(scale of e, scale of sigma2).  e_i = b_i - a_i x is formed to an absolute error of order n eps (||A||_F ||x|| + ||b||) =: n eps nrm
    however small it is, x being the exact solution of a problem within eps of the given one; with |de_i| <= d,
    |d sigma2| <= (2 sqrt(sum p e^2) sqrt(sum p) d + sum p d^2) / dof plus the rounding of the sum itself, m eps sigma2.  The second
    scale is that bound with d = nrm, its quadratic term dropped."""
    x, e = np.asarray(ref["x"], dtype=np.float64), np.asarray(ref["e"], dtype=np.float64)
    pq = np.ones(len(e)) if p is None else np.asarray(p, dtype=np.float64)
    incl = pq > 0
    nrm = np.linalg.norm(np.asarray(A)[incl]) * np.linalg.norm(x) + np.linalg.norm(np.asarray(b)[incl])
    dof = ref["dof"]
    if dof <= 0:
        return nrm, INF
    sig = float(ref["sigma2"])
    return nrm, 2.0 * np.sqrt((pq * e * e).sum()) * np.sqrt(pq.sum()) * nrm / dof + sig


def errors(out, ref):
    """the three measures of dict-like results against the reference (not yet divided by kappa eps)"""
    f = lambda v: np.asarray(v, dtype=np.float64)            # noqa: E731  (the differences are formed in the reference precision first)
    Cr, ser, hr = ref["C"], ref["se"], ref["h"]
    dC = f(H.norm(H.arr(out["C"]) - Cr)) / f(H.norm(Cr))
    dse = f(np.max(np.abs(H.arr(out["se"]) - ser))) / f(np.max(ser))
    dh = f(np.max(np.abs(H.arr(out["h"]) - hr))) if len(hr) else 0.0
    return {"C": float(dC), "se": float(dse), "h": float(dh)}


@functools.lru_cache(maxsize=None)
def reference_case(m, n, weighted, batch=BATCH):
    """per member: (the longdouble restatement, the float64 restatement, kappa) of make_case(m, n, weighted), unscaled (with_scale gives
    the scaled results); computed once and shared"""
    A, b, p = make_case(m, n, weighted, batch)
    out = []
    for q in range(batch):
        pq = None if p is None else p[q]
        out.append((fit_stats(A[q], b[q], pq, False, H.LD), fit_stats(A[q], b[q], pq, False, np.float64), kappa(A[q], pq)))
    return out


def rank_deficient_case(n, rank, batch, salt=0):
    """members of exact rank `rank` < n built as products with small integers: (n + 5) x n, float64"""
    rng = np.random.default_rng(8119000 + 100 * n + rank + 7 * salt)
    m = n + 5
    L = rng.integers(-3, 4, (batch, m, max(rank, 1))).astype(np.float64)
    Rt = rng.integers(-3, 4, (batch, max(rank, 1), n)).astype(np.float64)
    A = np.einsum("qik,qkj->qij", L, Rt)
    if rank == 0:
        A[:] = 0.0
    return A
