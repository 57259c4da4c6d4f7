"""A numpy restatement of the batched damped least squares (mi355x_qr.h section 8f; kernels: csrc/qr_batched_damped.hip) for one member,
with the inputs, the truth and the error measures of its tests (helper module, no fixtures, no GPU).

Straight loops, no LAPACK, parameterised by dtype like hp_ref.py and batched_update_ref.py.  step() eliminates the n rows of
S = lambda diag(d) against the triangle R with Z riding along: for j = 0 .. n-1, x = S(0..j, j), ssq = |x|^2; ssq == 0 touches nothing;
else beta = -sign(alpha) hypot(alpha, sqrt(ssq)), tau = (beta - alpha) / beta, v = x / (alpha - beta) and the later columns take the
reflector [e_j ; v].  solve() adds the back substitution, |D x| and sqrt(|R x - z|^2 + rss) from the untouched R and Z.  tall() and
wide() are the two-stage restatements (hp_ref's Householder QR, then solve()): their float64 instances are "the same operation in
working precision" that the GPU test measures the kernels against.

The truth is hp_ref.lstsq in longdouble on the stacked system [A ; lambda D] x = [b ; 0].

Measures per (member, lambda), evaluated in longdouble, the worst right-hand side:
  forward   |X - X_ld| / |X_ld|                          cap 50 (kappa + kappa^2 |r| / (|S| |X|)) eps on the stacked matrix S
                                                         (test_gpu_lstsq.py's least-squares perturbation bound)
  xnorm     | |D x| - |D x_ld| | / |D x_ld|              cap kappa(D) x the forward cap + rows(S) eps: | |D x| - |D x_ld| | <=
                                                         max d |x - x_ld| and |D x_ld| >= min d |x_ld|; the second term is the
                                                         rounding of the norm itself (a sum of at most rows(S) squares)
  resid     | rho - |A x_ld - b| | / |A x_ld - b|        cap the forward cap x |A|_2 |x_ld| / |A x_ld - b| + rows(S) eps: the residual
                                                         norm moves by at most |A|_2 |x - x_ld|; the norm's own rounding as above
  stacked   |S^T (S x - c)| / (|S|^2 |x| + |S| |c|)      cap 4 rows(S) eps: x solves a system perturbed by E, and this measure is at most
                                                         about 2 |E| / |S|; the two orthogonal stages (the QR, the elimination of the
                                                         block) each leave |E| / |S| at rows(S) eps (test_gpu_batched_minnorm.py's cap)
"""
import functools

import numpy as np

import hp_ref as H
from batched_update_ref import _hypot

LD = H.LD
EPS = H.EPS
BATCH = 9

# (m, n, nrhs): the shapes of tests/test_gpu_batched_damped.py -- the wave route at its register edge, the first shapes past each edge, the
# workgroup route up to the LDS limit, a composed factorisation
SHAPES = [(1, 1, 1), (5, 3, 2), (17, 17, 1), (64, 31, 1), (64, 28, 4), (64, 32, 1), (65, 4, 1), (100, 33, 2), (256, 63, 1), (300, 40, 3)]
# the wide members as the tall F they are the transposes of: (rows, cols) of F, the member is cols x rows
WIDE = [(7, 6), (2, 1), (31, 3), (64, 8), (100, 33), (300, 40)]
WIDE_NRHS = (1, 3)
# lambda in units of |A|_2; 0 only where m > n
LAMS = (0.0, 1e-8, 0.3, 30.0, 1e3)


def U(seed, *shape):
    return np.random.default_rng(seed).random(shape) - 0.5


def step(R, Z, sdiag, dtype=np.float64):
    """[R | Z] stacked on [diag(sdiag) | 0] -> (R~, z~); R and Z are not modified"""
    R0 = H.arr(np.triu(np.asarray(R)), dtype)
    n = R0.shape[0]
    T = np.hstack([R0, H.arr(Z, dtype)])
    M = H.arr(np.zeros(T.shape), dtype)
    sd = H.arr(sdiag, dtype)
    for j in range(n):
        M[j, j] = sd[j]
    for j in range(n):
        x = M[:j + 1, j].copy()
        ssq = (x * x).sum()
        if ssq == 0:
            continue
        alpha = T[j, j]
        h = _hypot(alpha, H._root(ssq, dtype), dtype)
        beta = -h if alpha >= 0 else h
        tau = (beta - alpha) / beta
        v = x / (alpha - beta)
        tw = tau * (T[j, j + 1:] + (v[:, None] * M[:j + 1, j + 1:]).sum(axis=0))
        T[j, j + 1:] = T[j, j + 1:] - tw
        M[:j + 1, j + 1:] = M[:j + 1, j + 1:] - v[:, None] * tw[None, :]
        T[j, j] = beta
    return T[:, :n], T[:, n:]


def solve(R, Z, lam, d=None, jpvt=None, rss=None, flip=False, dtype=np.float64):
    """one lambda from factors: (X in the caller's row order, |D x| per column, resid per column, info).  flip: the triangle is read as
    U(i, k) = R(n-1-k, n-1-i), Z and the rows of X reversed.  info != 0: X, xnorm and resid are None"""
    R0, Z0 = H.arr(np.triu(np.asarray(R)), dtype), H.arr(Z, dtype)
    n, nrhs = Z0.shape
    if flip:
        assert d is None and jpvt is None
        R0, Z0 = R0.T[::-1, ::-1].copy(), Z0[::-1].copy()
    jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
    dd = H.arr(np.ones(n) if d is None else np.asarray(d)[jp], dtype)
    Rt, zt = step(R0, Z0, H.arr(lam, dtype) * dd, dtype)
    for i in range(n):
        if Rt[i, i] == 0:
            return None, None, None, i + 1
    Xp = H.solve_r(Rt, zt, dtype)
    E = Xp * 0
    for c in range(n):                                    # R x - z from the untouched factors, the columns ascending
        E = E + R0[:, c][:, None] * Xp[c][None, :]
    E = E - Z0
    tail = H.arr(np.zeros(nrhs) if rss is None else rss, dtype)
    resid = np.array([H._root((E[:, k] * E[:, k]).sum() + tail[k], dtype) for k in range(nrhs)])
    DX = dd[:, None] * Xp
    xnorm = np.array([H._root((DX[:, k] * DX[:, k]).sum(), dtype) for k in range(nrhs)])
    X = Xp * 0
    X[(n - 1 - np.arange(n)) if flip else jp] = Xp
    return X, xnorm, resid, 0


def tall(A, B, lams, d=None, dtype=np.float64):
    """the two-stage restatement for m >= n: Householder QR, Q^T B, then solve() per lambda: a list of (X, xnorm, resid, info)"""
    F, tau = H.qr(A, dtype)
    n = F.shape[1]
    QtB = H.apply_q(F, tau, B, "T", dtype)
    rss = (QtB[n:] * QtB[n:]).sum(axis=0)
    return [solve(H.triu(F), QtB[:n], lam, d, None, rss, False, dtype) for lam in lams]


def wide(A, B, lams, dtype=np.float64):
    """m < n, D = I: A^T = Q R, y from the flipped triangle, x = Q [y ; 0]"""
    A = H.arr(A, dtype)
    m, n = A.shape
    F, tau = H.qr(A.T.copy(), dtype)
    out = []
    for lam in lams:
        Y, xnorm, resid, info = solve(H.triu(F), B, lam, None, None, None, True, dtype)
        if info:
            out.append((None, None, None, info))
            continue
        Y0 = H.arr(np.zeros((n, Y.shape[1])), dtype)
        Y0[:m] = Y
        out.append((H.apply_q(F, tau, Y0, "N", dtype), xnorm, resid, 0))
    return out


def stacked(A, lam, d=None):
    """[A ; lam diag(d)] in longdouble"""
    n = np.shape(A)[1]
    dd = H.arr(np.ones(n) if d is None else d)
    S = H.arr(np.zeros((n, n)))
    for i in range(n):
        S[i, i] = H.arr(lam) * dd[i]
    return np.vstack([H.arr(A), S])


def truth(A, B, lam, d=None):
    """(X, |D x|, |A x - b|) in longdouble from the stacked system"""
    n = np.shape(A)[1]
    S = stacked(A, lam, d)
    X, _ = H.lstsq(S, np.vstack([H.arr(B), H.arr(np.zeros((n, np.shape(B)[1])))]))
    dd = H.arr(np.ones(n) if d is None else d)
    DX, E = dd[:, None] * X, H.matmul(A, X) - H.arr(B)
    cols = range(X.shape[1])
    return X, np.array([H.norm(DX[:, k]) for k in cols]), np.array([H.norm(E[:, k]) for k in cols])


def measures(A, B, lam, d, X, xnorm, resid, T):
    """(forward, xnorm, resid, stacked) of one (member, lambda) against the truth T = truth(...)"""
    Xld, xn, rs = T
    X = H.arr(X)
    fwd = float(H.norm(X - Xld) / H.norm(Xld))
    exn = float(max(abs(H.arr(xnorm) - xn) / xn))
    ers = float(max(abs(H.arr(resid) - rs) / rs))
    S = stacked(A, lam, d)
    C = np.vstack([H.arr(B), H.arr(np.zeros(X.shape))])
    return fwd, exn, ers, float(H.normal_equations_residual(S, X, C))


def caps(A, B, lam, d, T):
    Xld, xn, rs = T
    S = np.asarray(stacked(A, lam, d), dtype=np.float64)
    sv = np.linalg.svd(S, compute_uv=False)
    kappa, s2 = sv[0] / sv[-1], sv[0]
    n = S.shape[1]
    C = np.vstack([np.asarray(B, dtype=np.float64), np.zeros((n, np.shape(B)[1]))])
    X64 = np.asarray(Xld, dtype=np.float64)
    rn = np.linalg.norm(S @ X64 - C)
    fcap = 50.0 * (kappa + kappa ** 2 * rn / (s2 * np.linalg.norm(X64))) * EPS
    dd = np.ones(n) if d is None else np.abs(np.asarray(d))
    a2 = np.linalg.norm(np.asarray(A, dtype=np.float64), 2)
    xl = np.array([float(H.norm(Xld[:, k])) for k in range(X64.shape[1])])
    rcap = fcap * float(max(a2 * xl / np.asarray(rs, dtype=np.float64)))
    own = S.shape[0] * EPS                                # the rounding of a norm of at most rows(S) terms, in its own right
    return fcap, fcap * dd.max() / dd.min() + own, rcap + own, 4 * S.shape[0] * EPS


NAMES = ("forward", "xnorm", "resid", "stacked")


def lam_list(A, m, n):
    """the lambdas of a member: LAMS x |A|_2, 0 only where m > n"""
    a2 = np.linalg.norm(A, 2)
    return np.array([l * a2 for l in LAMS if l > 0 or m > n])


@functools.lru_cache(maxsize=None)
def case(m, n, nrhs, with_d=True, batch=None, salt=0):
    """`batch` (default: 9 up to 64 x 32, 5 above: the longdouble truth is the cost of this file) seeded members of m x n (tall: m >= n; wide: m < n and no d): A, B, d (uniform in [0.5, 2] or None), lam (batch, nlam),
    and per member and lambda the truth, the float64 two-stage restatement's measures and the caps"""
    batch = batch or (BATCH if m * n <= 64 * 32 else 5)
    seed = 1000 * m + 10 * n + nrhs + 77777 * salt
    A, B = U(seed, batch, m, n), U(seed + 500000, batch, m, nrhs)
    d = (0.5 + 1.5 * np.random.default_rng(seed + 900000).random((batch, n))) if with_d else None
    lam = np.stack([lam_list(A[q], m, n) for q in range(batch)])
    T, ref, cp = [], [], []
    for q in range(batch):
        dq = None if d is None else d[q]
        r64 = tall(A[q], B[q], lam[q], dq) if m >= n else wide(A[q], B[q], lam[q])
        Tq, rq, cq = [], [], []
        for k, l in enumerate(lam[q]):
            t = truth(A[q], B[q], l, dq)
            X, xn, rs, info = r64[k]
            assert info == 0
            Tq.append(t)
            rq.append(measures(A[q], B[q], l, dq, X, xn, rs, t))
            cq.append(caps(A[q], B[q], l, dq, t))
        T.append(Tq); ref.append(rq); cp.append(cq)
    for x in (A, B, lam) + (() if d is None else (d,)):
        x.setflags(write=False)
    return dict(A=A, B=B, d=d, lam=lam, T=T, ref=ref, caps=cp)
