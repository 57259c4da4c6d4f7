"""A numpy restatement of the batched signed-row update (mi355x_qr.h section 8d; kernels: csrc/qr_batched_update.hip) for one member.

Straight loops over the columns, no LAPACK, parameterised by dtype like hp_ref.py: the longdouble instance is the reference, the float64
instance of the very same code is "the same operation in working precision" that the GPU test measures the kernels against.  Per column,
with sa / sd the sums of squares of the added / removed rows: h = hypot(alpha, sqrt(sa)), nd = sqrt(sd), d = (h - nd)(h + nd) -- the
difference of squares is never formed --, beta = -sign(alpha) sqrt(d), tau = (beta - alpha) / beta, v = b / (alpha - beta); an exactly
zero block column gives tau = 0 and touches nothing; d <= 0 or not finite is the failure, reported as the column + 1 with every input
returned as it came.  Reflector j is I - tau_j u_j u_j^T Phi with u_j = [e_j ; v_j], Phi = diag(I, S): only the products that contract
over the block's rows see the signs.  Sums are plain `(x * x).sum()`: for a power of two s every function here is exactly homogeneous
while nothing leaves the normal range.
"""
import numpy as np

import hp_ref as H

LD = H.LD
EPS = H.EPS


def _hypot(a, b, dtype):
    """sqrt(a^2 + b^2) without forming the squares where the platform has the function (the kernels call hypot)"""
    if dtype is LD and H._lift is not None:
        return H._root(a * a + b * b, dtype)
    return np.hypot(a, b)


def _finite(x):
    return bool(np.isfinite(np.float64(x)))


def update(R, B, p_add, C1=None, C2=None, dtype=np.float64):
    """[R ; B] -> [R' ; 0] with the first p_add rows of B added and the rest removed; [C1 ; C2] ride along.
    Returns (R', V, tau, C1', C2', info): info = 0, or the failing column + 1 with R, B, zeros, C1, C2 unchanged."""
    R0, B0 = H.arr(np.triu(np.asarray(R)), dtype), H.arr(B, dtype)
    n, p = R0.shape[0], B0.shape[0]
    nrhs = 0 if C1 is None else np.shape(C1)[1]
    Z0 = H.arr(C1 if nrhs else np.zeros((n, 0)), dtype)
    E0 = H.arr(C2 if nrhs else np.zeros((p, 0)), dtype)
    Rw, Bw, Zw, Ew = R0.copy(), B0.copy(), Z0.copy(), E0.copy()
    tau = H.arr(np.zeros(n), dtype)
    s = H.arr(np.where(np.arange(p) < p_add, 1.0, -1.0), dtype)
    T = np.hstack([Rw, Zw])                              # [R | Z] and [B | C2]: the right-hand sides are columns n .. of the same loop
    M = np.hstack([Bw, Ew])
    for j in range(n):
        b = M[:, j]
        sa, sd = (b[:p_add] * b[:p_add]).sum(), (b[p_add:] * b[p_add:]).sum()
        if sa == 0 and sd == 0:
            continue
        alpha = T[j, j]
        h, nd = _hypot(alpha, H._root(sa, dtype), dtype), H._root(sd, dtype)
        d = (h - nd) * (h + nd)
        if not (d > 0) or not _finite(d):
            return R0, B0, H.arr(np.zeros(n), dtype), Z0, E0, j + 1
        beta = -H._root(d, dtype) if alpha >= 0 else H._root(d, dtype)
        tau[j] = (beta - alpha) / beta
        v = b / (alpha - beta)
        tw = tau[j] * (T[j, j + 1:] + ((s * v)[:, None] * M[:, j + 1:]).sum(axis=0))      # every later column, one after the other
        T[j, j + 1:] = T[j, j + 1:] - tw
        M[:, j + 1:] = M[:, j + 1:] - v[:, None] * tw[None, :]
        M[:, j] = v
        T[j, j] = beta
    Rw, Zw, Bw, Ew = T[:, :n], T[:, n:], M[:, :n], M[:, n:]
    return Rw, Bw, tau, Zw, Ew, 0


def apply(V, tau, p_add, C1, C2, dtype=np.float64):
    """[C1 ; C2] <- Theta_{n-1} .. Theta_0 [C1 ; C2] with the reflectors of update()"""
    V, tau, Z, E = H.arr(V, dtype), H.arr(tau, dtype), H.arr(C1, dtype), H.arr(C2, dtype)
    p, n = V.shape
    s = H.arr(np.where(np.arange(p) < p_add, 1.0, -1.0), dtype)
    for j in range(n):
        if tau[j] == 0:
            continue
        tw = tau[j] * (Z[j] + ((s * V[:, j])[:, None] * E).sum(axis=0))
        Z[j] = Z[j] - tw
        E[:] = E - V[:, j][:, None] * tw[None, :]
    return Z, E


class Accumulator:
    """one member of qr_lsacc_batched: R, Z, the residual sums and the row count; step() is push (p_del = 0), pop (p_add = 0) or slide"""

    def __init__(self, n, nrhs, dtype=np.float64):
        self.n, self.nrhs, self.dtype = n, nrhs, dtype
        self.R, self.Z = H.arr(np.zeros((n, n)), dtype), H.arr(np.zeros((n, nrhs)), dtype)
        self.rss, self.rows = H.arr(np.zeros(nrhs), dtype), 0

    def step(self, Anew, Bnew, Aold, Bold):
        """returns info: 0, the failing column + 1, or -1 when fewer than n rows would be left; non-zero: the state is as it was"""
        p_add, p_del = len(Anew), len(Aold)
        if p_del > 0 and self.rows + p_add - p_del < self.n:
            return -1
        blk = np.vstack([np.asarray(Anew).reshape(p_add, self.n), np.asarray(Aold).reshape(p_del, self.n)])
        rhs = np.vstack([np.asarray(Bnew).reshape(p_add, self.nrhs), np.asarray(Bold).reshape(p_del, self.nrhs)])
        R, _, _, Z, E, info = update(self.R, blk, p_add, self.Z, rhs, self.dtype)
        if info:
            return info
        ea, ed = (E[:p_add] * E[:p_add]).sum(axis=0), (E[p_add:] * E[p_add:]).sum(axis=0)
        rss = (self.rss + ea) - ed
        self.R, self.Z, self.rss = R, Z, np.where(rss > 0, rss, rss * 0)
        self.rows += p_add - p_del
        return 0


def measures(n, p_add, m, Rn, C1n, C2n, Rld):
    """the three ratios to their bounds for one member's results"""
    p = m["B"].shape[0]
    S = np.where(np.arange(p) < p_add, 1.0, -1.0)[:, None]
    G0 = m["R"].T @ m["R"]
    g = np.linalg.norm(Rn.T @ Rn - (G0 + m["B"].T @ (S * m["B"]))) / np.linalg.norm(G0) / (n * EPS)
    kappa = np.linalg.cond(Rn)
    e = float(H.norm(H.arr(Rn) - Rld) / H.norm(Rld)) / (50 * kappa * EPS)
    inv = 0.0
    if m["C1"].shape[1]:
        before = (m["C1"] ** 2).sum(axis=0) + (S * m["C2"] ** 2).sum(axis=0)
        after = (C1n ** 2).sum(axis=0) + (S * C2n ** 2).sum(axis=0)
        inv = np.max(np.abs(after - before) / ((m["C1"] ** 2).sum(axis=0) + (m["C2"] ** 2).sum(axis=0))) / ((n + p) * EPS)
    return g, e, inv
