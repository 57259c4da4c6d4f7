"""Inputs, references and error measures of the batched equality-constrained least-squares tests (mi355x_qr.h section 8h; helper module, no
fixtures, no GPU).

A case is (m, n, p, nrhs): `batch` members min ||A x - b|| subject to C x = d with A m x n, C p x n, b m x nrhs, d p x nrhs, entries
standard normal from numpy's default_rng(seed).  Every third member (q % 3 == 1) has A's columns graded to condition 1e6, every third
member offset by one (q % 3 == 2) has C's rows graded to 1e6.

`gglse` restates the eight steps of the header's section 8h on hp_ref's qr, apply_q, solve_r and solve_rt; its longdouble instance is the
reference, its float64 instance "the same operation in working precision" that the GPU test measures the kernels against.

Measures per member and right-hand side, all evaluated in longdouble:
    constraint   ||C x - d|| / (||C||_F ||x|| + ||d||)                                              cap (n + 8) eps
    kkt          ||A^T (A x - b) + C^T lam|| / (||A||_2 (||A||_2 ||x|| + ||b||) + ||C||_2 ||lam||)  cap (n + 8) eps
    residual     |resid - ||A x - b||| / (||A||_F ||x|| + ||b||)                                    cap (m + n) eps
    forward      ||x - x_ld|| / ||x_ld||                                                            cap 50 kappa eps
with kappa = kappa_2(C) (1 + ||A||_2 / sigma_min(A Z)) + kappa_2(A Z) + kappa_2(A Z)^2 ||A x - b|| / (||A||_2 ||x||), Z the last n - p
columns of the complete Q of C^T (kappa_2(A Z) = sigma_min = 1 when p == n).
"""
import functools

import numpy as np

import hp_ref as H

EPS = H.EPS
BATCH = 9
NAMES = ("constraint", "kkt", "residual", "forward")

# (m, n, p, nrhs): the shapes of tests/test_gpu_batched_lse.py, wave route then workgroup route
WAVE_SHAPES = [(1, 1, 1, 1), (1, 2, 1, 1), (3, 2, 1, 1), (2, 3, 2, 1), (8, 5, 5, 2), (16, 8, 3, 1), (64, 31, 7, 1), (64, 20, 19, 3)]
WG_SHAPES = [(65, 31, 7, 1), (40, 32, 31, 1), (100, 33, 10, 1), (256, 40, 12, 2), (130, 63, 20, 1), (30, 63, 40, 1), (200, 30, 1, 2)]
SHAPES = WAVE_SHAPES + WG_SHAPES


def gglse(A, C, B, D, dtype=H.LD):
    """(X, lam, resid) of min ||A x - b|| subject to C x = d, every column of (B, D) a pair, by the null-space method in `dtype`"""
    A, C, B, D = H.arr(A, dtype), H.arr(C, dtype), H.arr(B, dtype), H.arr(D, dtype)
    n = A.shape[1]
    p = C.shape[0]
    k = n - p
    Fc, tc = H.qr(C.T, dtype)                                 # 1. C^T = Q_c [R_c ; 0]
    Rc = H.triu(Fc)
    Y1 = H.solve_rt(Rc, D, dtype)                             # 2. R_c^T y1 = d
    At = H.apply_q(Fc, tc, A.T, "T", dtype).T                 # 3. A Q_c = (Q_c^T A^T)^T
    R = B.copy()                                              # 4. r = b - A~1 y1
    for i in range(p):
        R -= At[:, i][:, None] * Y1[i][None, :]
    Fa, ta = H.qr(At[:, p:], dtype)                           # 5. the QR of A~2; r and A~1 ride along
    T = H.apply_q(Fa, ta, R, "T", dtype)
    G = H.apply_q(Fa, ta, At[:, :p], "T", dtype)
    Y2 = H.solve_r(H.triu(Fa), T[:k], dtype)
    X = H.apply_q(Fc, tc, np.concatenate([Y1, Y2]), "N", dtype)        # 6. x = Q_c [y1 ; y2]
    resid = H.arr(np.zeros(B.shape[1]), dtype)                # 7. resid = ||t(n-p : m)||
    g = H.arr(np.zeros((p, B.shape[1])), dtype)               # 8. R_c lam = g
    for j in range(B.shape[1]):
        resid[j] = H.norm(T[k:, j], dtype)
        for r in range(k, T.shape[0]):
            g[:, j] += G[r] * T[r, j]
    lam = H.solve_r(Rc, g, dtype)
    return X, lam, resid


def graded(rng, rows, cols, axis, cond=1e6):
    """standard normal with the columns (axis 1) or rows (axis 0) graded from 1 down to 1 / cond"""
    M = rng.standard_normal((rows, cols))
    s = np.logspace(0, -np.log10(cond), M.shape[axis])
    return M * (s[None, :] if axis == 1 else s[:, None])


def member(m, n, p, nrhs, q, seed):
    rng = np.random.default_rng(seed)
    A = graded(rng, m, n, 1) if q % 3 == 1 else rng.standard_normal((m, n))
    C = graded(rng, p, n, 0) if q % 3 == 2 else rng.standard_normal((p, n))
    return A, C, rng.standard_normal((m, nrhs)), rng.standard_normal((p, nrhs))


def kappa_parts(A, C):
    """(kappa_2(C), kappa_2(A Z), sigma_min(A Z), ||A||_2) of the forward bound (module docstring)"""
    n = A.shape[1]
    p = C.shape[0]
    sc = np.linalg.svd(C, compute_uv=False)
    kz, smin = 1.0, 1.0
    if p < n:
        Z = np.linalg.qr(C.T, mode="complete")[0][:, p:]
        sz = np.linalg.svd(A @ Z, compute_uv=False)
        kz, smin = sz[0] / sz[-1], sz[-1]
    return sc[0] / sc[-1], kz, smin, np.linalg.norm(A, 2)


def caps(A, C, B, Xld):
    """per right-hand side (constraint, kkt, residual, forward) caps"""
    m, n = A.shape
    kc, kz, smin, nA = kappa_parts(A, C)
    Rl = H.matmul(A, Xld) - H.arr(B)
    out = []
    for j in range(B.shape[1]):
        kap = kc * (1.0 + nA / smin) + kz + kz * kz * float(H.norm(Rl[:, j])) / (nA * float(H.norm(Xld[:, j])))
        out.append(((n + 8) * EPS, (n + 8) * EPS, (m + n) * EPS, 50.0 * kap * EPS))
    return out


def measures(A, C, B, D, X, lam, resid, Xld):
    """per right-hand side (constraint, kkt, residual, forward), evaluated in longdouble; lam or resid may be None (their measure is 0)"""
    Al, Cl, Bl, Dl, Xl = H.arr(A), H.arr(C), H.arr(B), H.arr(D), H.arr(X)
    nA2, nC2 = np.linalg.norm(A, 2), np.linalg.norm(C, 2)
    nAF, nCF = float(H.norm(Al)), float(H.norm(Cl))
    Rl = H.matmul(Al, Xl) - Bl
    Ec = H.matmul(Cl, Xl) - Dl
    out = []
    for j in range(B.shape[1]):
        nx, nb = float(H.norm(Xl[:, j])), float(H.norm(Bl[:, j]))
        con = float(H.norm(Ec[:, j])) / (nCF * nx + float(H.norm(Dl[:, j])))
        kkt = 0.0
        if lam is not None:
            Ll = H.arr(lam)[:, j:j + 1]
            gk = H.matmul(Al.T, Rl[:, j:j + 1]) + H.matmul(Cl.T, Ll)
            kkt = float(H.norm(gk)) / (nA2 * (nA2 * nx + nb) + nC2 * float(H.norm(Ll)))
        res = 0.0
        if resid is not None:
            res = float(abs(H.arr(resid)[j] - H.norm(Rl[:, j]))) / (nAF * nx + nb)
        fwd = float(H.norm(Xl[:, j] - H.arr(Xld)[:, j]) / H.norm(H.arr(Xld)[:, j]))
        out.append((con, kkt, res, fwd))
    return out


@functools.lru_cache(maxsize=None)
def case(m, n, p, nrhs, batch=BATCH, salt=0):
    """`batch` members: A (batch, m, n), C (batch, p, n), B (batch, m, nrhs), D (batch, p, nrhs), read-only, and per member Xld, lamld,
    residld (the longdouble instance), ref (the float64 instance's measures per right-hand side) and caps"""
    mem = [member(m, n, p, nrhs, q, 100000 * m + 1000 * n + 10 * p + nrhs + 7919 * q + 77777 * salt) for q in range(batch)]
    out = dict(Xld=[], lamld=[], residld=[], X64=[], ref=[], caps=[])
    for A, C, B, D in mem:
        Xl, ll, rl = gglse(A, C, B, D)
        X6, l6, r6 = gglse(A, C, B, D, np.float64)
        out["Xld"].append(Xl); out["lamld"].append(ll); out["residld"].append(rl); out["X64"].append(X6)
        out["ref"].append(measures(A, C, B, D, X6, l6, r6, Xl))
        out["caps"].append(caps(A, C, B, Xl))
    for key, idx in (("A", 0), ("C", 1), ("B", 2), ("D", 3)):
        out[key] = np.stack([x[idx] for x in mem])
        out[key].setflags(write=False)
    return out
