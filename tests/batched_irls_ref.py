"""Inputs, the restatement and the error measures of the batched robust and weighted least-squares tests (mi355x_qr.h section 8j; helper
module, no fixtures, no GPU).

`irls` restates the five steps of the header's section 8j in straight loops, parametrised by dtype; every solve is hp_ref.lstsq's own
steps (qr, apply_q, solve_r: no LAPACK), taken apart only to see an exactly zero R(i,i).  Its float64 instance is "the same operation in
working precision" that the GPU test measures the kernels against; its longdouble instance is the reference.  The kernels take the same
decisions in the same order.  The float64 instance forms the residual with one fused multiply-add per term, as the kernels do (`fma64`
below: numpy has none), so that an exactly zero residual -- the only decision that rests on single bits -- is zero in both.  `solves=k`
is the fixed-iteration mode: the stopping test is recorded, never taken, and exactly k solves run; the accuracy comparison runs the
longdouble instance for the number of solves the float64 instance took.

A case is (m, n, loss): `batch` planted members
    A        standard normal m x n from numpy's default_rng(seed); every third member (q % 3 == 1) has its columns graded to 1e4, with x*
             scaled inversely
    b        A x* + 0.01 noise, then k = max(0, min(m // 5, (m - n) // 3)) rows shifted by +-[10, 50] x 0.01: the planted outliers

Measures per member against the longdouble instance (xl, sl, wl), D the column norms of A, nrm = ||A||_F ||xl|| + ||b||:
    x   ||D (x - xl)|| / ||D xl||        s   |s - sl| / nrm        w   max_i |w_i - wl_i| sl / nrm
each capped at 50 kappa eps, kappa the condition of diag(sqrt(c)) A with unit-norm columns at the final weights c = p wl.  s is a
residual, and a residual is computed to an absolute error of about eps nrm however small it is against b (here 0.01 against about
sqrt(n)), so its error is taken against nrm, not against s; w_i is a function of r_i / s whose slope is at most about 1 / (tune s), so an
error of w_i times s is again a residual's error and is taken against nrm.
"""
import functools

import numpy as np

import hp_ref as H

EPS = H.EPS
BATCH = 9
NAMES = ("x", "s", "w")
INF = np.inf
LS, HUBER, BISQUARE = 0, 1, 2
LOSS_NAMES = {LS: "ls", HUBER: "huber", BISQUARE: "bisquare"}
MAD = 0.6744897501960817
DEFAULT_TUNE = {LS: 1.0, HUBER: 1.345, BISQUARE: 4.685}
TOL = 1e-6

# (m, n): the shapes of tests/test_gpu_batched_irls.py, wave route then workgroup route (the last: qr_irls_batched_max_rows(63) x 63)
WAVE_SHAPES = [(1, 1), (3, 2), (8, 2), (16, 7), (64, 7), (64, 15), (64, 31)]
MAX_ROWS_63 = 290
WG_SHAPES = [(65, 15), (40, 32), (100, 20), (256, 40), (MAX_ROWS_63, 63)]
SHAPES = WAVE_SHAPES + WG_SHAPES

# (m, n, loss) -> the salt of that case's seeds (test_batched_irls_ref.py).  16 x 7 Huber: a deciding change lies at 1.006 tol at salt 0
# and at 1.001 tol at salt 1 (none within 3 % at salt 3).  65 x 15: at salt 0 member 1 does not settle within 50 solves and leaves a planted row at Huber weight 0.67 (one member
# in about three hundred over salts 0 to 5; the recovery conditions describe members that converge)
SALT = {(16, 7, HUBER): 3, (65, 15, HUBER): 1, (65, 15, BISQUARE): 1}


def losses(m, n):
    """the robust losses run at a shape: bisquare only where m >= 2 n (below, the weights can collapse and the precisions part ways)"""
    return (HUBER, BISQUARE) if m >= 2 * n else (HUBER,)


def recovers(m, n):
    """the shapes on which the recovery conditions are asserted"""
    return m >= 4 * n and m >= 32


def max_rows(n):
    """qr_irls_batched_max_rows from its byte formula: the largest m <= 512 with 8 ((n + 1) ld(m) + 3 m + 2 n + 72) <= 160 KiB"""
    if n < 1 or n > 63:
        return 0
    m = 512
    while m >= n and 8 * ((n + 1) * (((m + 29) // 32) * 32 + 2) + 3 * m + 2 * n + 72) > 160 * 1024:
        m -= 1
    return m if m >= n else 0


def _split(a):
    t = 134217729.0 * a
    hi = t - (t - a)
    return hi, a - hi


def fma64(a, b, c):
    """a * b + c with one rounding, elementwise on float64 (Dekker's exact product, Knuth's exact sum; the last two additions can round
    twice in rare cases, an exact zero is always exact)"""
    a, b, c = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64)
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def median_by_ranks(v):
    """the median of a 1-D array by the rank rule: rank_i = #{j : v_j < v_i, or v_j == v_i and j < i}; half the sum of the values of
    ranks (cnt - 1) // 2 and cnt // 2.  A NaN among them, or no value at all: NaN"""
    v = np.asarray(v)
    cnt = len(v)
    if cnt == 0 or any(x != x for x in v):
        return v.dtype.type(np.nan) if v.dtype != object else np.nan
    idx = np.arange(cnt)
    before = (v[None, :] < v[:, None]) | ((v[None, :] == v[:, None]) & (idx[None, :] < idx[:, None]))
    rank = before.sum(axis=1)
    v1 = v[int(np.flatnonzero(rank == (cnt - 1) // 2)[0])]
    v2 = v[int(np.flatnonzero(rank == cnt // 2)[0])]
    return (v1 + v2) / 2


def weight(loss, u, k):
    """the robust weights of u = |r| / s"""
    with np.errstate(divide="ignore", invalid="ignore"):
        if loss == HUBER:
            return np.where(u <= k, 1 + 0 * k, k / u)
        t = u / k
        h = 1 - t * t
        return np.where(u < k, h * h, 0 * k)


def residual(A, b, x, dtype=np.float64):
    """r = b - A x, the columns in ascending order, one fused multiply-add per term in float64"""
    r = b.copy()
    for j in range(A.shape[1]):
        r = fma64(-A[:, j], x[j], r) if dtype is np.float64 else r - A[:, j] * x[j]
    return r


def irls(A, b, loss, tune=0.0, prior=None, scale=None, x0=None, tol=1e-8, maxit=0, dtype=np.float64, solves=None):
    """dict(x, w, s, resid, iter, status, info, changes) of the fit of section 8j in `dtype`; everything but info is None where the call
    writes nothing (info -1, -2 or i + 1).  changes: max_j |x_j - xold_j| / max_j |x_j| of every stopping test, in order"""
    m, n = np.shape(A)
    nothing = dict(x=None, w=None, s=None, resid=None, iter=None, status=None, changes=[])
    p64 = np.ones(m) if prior is None else np.asarray(prior, dtype=np.float64)
    # 1. the checks
    for i in range(m):
        if not (p64[i] >= 0 and p64[i] < INF):
            return dict(nothing, info=-1)
    if scale is not None and not (scale > 0 and scale < INF):
        return dict(nothing, info=-1)
    incl = p64 > 0
    A = H.arr(np.where(incl[:, None], A, 0.0), dtype)         # an excluded row is zeros whatever it holds
    b = H.arr(np.where(incl, b, 0.0), dtype)
    p = H.arr(p64, dtype)
    one = H.arr(np.ones(m), dtype)
    k = H.arr(np.float64(tune if tune > 0 else DEFAULT_TUNE[loss]), dtype)
    maxit = 50 if maxit <= 0 else maxit
    if solves is not None:
        maxit = solves
    robust = loss != LS
    # 2. the start
    w, it, status = one.copy(), 0, 0
    s = H.arr(np.float64(0.0), dtype)
    havex = robust and x0 is not None
    x = H.arr(x0, dtype) if havex else None
    xold = x.copy() if havex else None
    haveold, solved = havex, False
    changes = []
    r = None
    while True:
        if havex:
            # 4. the residual of x, the scale and the weights
            r = residual(A, b, x, dtype)
            if not robust:
                break
            v = abs(r)
            s = H.arr(np.float64(scale), dtype) if scale is not None else median_by_ranks(v[incl]) / H.arr(np.float64(MAD), dtype)
            if s == 0:
                status, w = 2, one.copy()
                break
            w = weight(loss, v / s, k)
            # 5. the stopping test
            if solved and haveold:
                xm, d = max(abs(x)), max(abs(x - xold))
                if d == d and xm == xm:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        changes.append(float(d / xm) if xm != 0 else (0.0 if d == 0 else INF))
                    if solves is None and d <= tol * xm:
                        break
            xold, haveold = x.copy(), True
        # 3. one solve
        c = p * w
        if int(np.sum(incl & np.array([ci > 0 for ci in c]))) < n:
            return dict(nothing, info=-2)
        if it == maxit:
            status = 3
            break
        it += 1
        sq = np.where(incl, H._root(np.where(incl, c, 0 * c), dtype), 0 * c)
        F, tau = H.qr(A * sq[:, None], dtype)
        for i in range(n):
            if F[i, i] == 0:
                return dict(nothing, info=i + 1)
        y = H.apply_q(F, tau, b * sq, "T", dtype)
        x = H.solve_r(H.triu(F), y[:n], dtype)
        solved = havex = True
    return dict(x=x, w=w, s=s, resid=H.norm(r, dtype), iter=it, status=status, info=0, changes=changes)


def planted_count(m, n):
    return max(0, min(m // 5, (m - n) // 3))


def member(m, n, q, seed):
    """one planted member: (A, b, xstar, rows) with rows the planted outliers"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    xs = rng.standard_normal(n)
    if q % 3 == 1:
        g = np.logspace(0, -4, n)
        A, xs = A * g[None, :], xs / g
    b = A @ xs + 0.01 * rng.standard_normal(m)
    k = planted_count(m, n)
    rows = np.sort(rng.choice(m, size=k, replace=False))
    b[rows] += rng.choice([-1.0, 1.0], size=k) * rng.uniform(10.0, 50.0, size=k) * 0.01
    return A, b, xs, rows


def scaled_error(A, x, xref):
    """||D (x - xref)|| / ||D xref|| in longdouble, D the column norms of A"""
    d = H.arr(np.linalg.norm(A, axis=0))
    return float(H.norm(d * (H.arr(x) - H.arr(xref))) / H.norm(d * H.arr(xref)))


def measures(A, b, x, s, w, ref):
    """(x, s, w) errors of a float64 result against the longdouble result `ref`"""
    ex = scaled_error(A, x, ref["x"])
    sl = ref["s"]
    nrm = float(H.norm(A)) * float(H.norm(ref["x"])) + float(H.norm(b))
    es = float(abs(H.arr(np.float64(s)) - sl)) / nrm
    ew = float(max(abs(H.arr(w) - ref["w"]))) * float(sl) / nrm
    return ex, es, ew


def kappa(A, c):
    """the condition of diag(sqrt(c)) A with unit-norm columns"""
    M = np.sqrt(np.asarray(c, dtype=np.float64))[:, None] * A
    return float(np.linalg.cond(M / np.linalg.norm(M, axis=0)[None, :]))


def seed(m, n, q, salt):
    return 100000 * m + 1000 * n + 7919 * q + 77777 * salt + 11


@functools.lru_cache(maxsize=None)
def members(m, n, salt=0, batch=BATCH):
    """`batch` planted members: A (batch, m, n), b (batch, m), xstar (batch, n), read-only, and rows (a list of index arrays)"""
    mem = [member(m, n, q, seed(m, n, q, salt)) for q in range(batch)]
    out = dict(rows=[x[3] for x in mem])
    for key, idx in (("A", 0), ("b", 1), ("xstar", 2)):
        out[key] = np.stack([x[idx] for x in mem])
        out[key].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(m, n, loss, batch=BATCH):
    """the members of (m, n) under SALT and per member: out64 (the float64 instance at TOL), outld (the longdouble instance run for out64's
    number of solves), ref (the measures of the float64 instance run for that number of solves, against outld) and cap (50 kappa eps)"""
    mem = members(m, n, SALT.get((m, n, loss), 0), batch)
    out = dict(mem, out64=[], outld=[], ref=[], cap=[])
    for q in range(batch):
        A, b = mem["A"][q], mem["b"][q]
        o = irls(A, b, loss, tol=TOL)
        assert o["info"] == 0
        old = irls(A, b, loss, solves=o["iter"], dtype=H.LD)
        out["out64"].append(o)
        out["outld"].append(old)
        out["ref"].append(measures(A, b, o["x"], o["s"], o["w"], old))          # (o left after o["iter"] solves: the fixed mode's own state)
        out["cap"].append(50 * kappa(A, np.asarray(old["w"], dtype=np.float64)) * EPS)
    return out


def estimating_equation(A, p, w, x, b):
    """||A^T (p o w o r)|| / (||A||_F ||p o w o r||) in longdouble, r = b - A x"""
    Al, xl = H.arr(A), H.arr(x)
    r = H.arr(b) - H.matmul(Al, xl[:, None])[:, 0]
    g = H.arr(p) * H.arr(w) * r
    return float(H.norm(H.matmul(Al.T, g[:, None])[:, 0]) / (H.norm(Al) * H.norm(g)))
