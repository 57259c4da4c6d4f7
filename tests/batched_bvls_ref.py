"""Inputs, the restatement and the error measures of the batched bound-constrained least-squares tests (mi355x_qr.h section 8i; helper
module, no fixtures, no GPU).

`bvls` restates the six steps of the header's section 8i in straight loops on hp_ref's qr, apply_q and solve_r (no LAPACK in the
elimination); its float64 instance is "the same operation in working precision" that the GPU test measures the kernels against.  The
kernels take the same decisions in the same order.

A case is (m, n): `batch` planted members min ||A x - b|| subject to lo <= x <= hi whose solution x* and active set are known exactly, so
that no test depends on the path the restatement takes:
    A        standard normal m x n from numpy's default_rng(seed); every third member (q % 3 == 1) has its columns graded to 1e4
    bounds   lo_j in -[0.5, 1.5], hi_j in +[0.5, 1.5]
    kinds    each variable is drawn free (x*_j in [-0.4, 0.4]; a quarter of these lose lo, a quarter hi, a quarter both, to infinity), at
             lo with multiplier w*_j = -u ||a_j|| or at hi with w*_j = +u ||a_j||, u in [0.5, 1.5]: about half the variables are active
    b        A x* + r with r = A (A^T A)^-1 w* (formed as Q R^-T w*) plus a random vector orthogonal to range(A): A^T r = w*
Strict complementarity and full column rank make x* and the state unique.

Measures per member, all evaluated in longdouble from the returned x, with nrm = ||A||_F ||x|| + ||b||:
    stationarity   max over free j of |a_j^T (b - A x)| / (||a_j|| nrm)
    w              max over j of |w_j - a_j^T (b - A x)| / (||a_j|| nrm)
    resid          |resid - ||A x - b||| / ||b||
each capped at (m + n) eps.
"""
import functools

import numpy as np

import hp_ref as H

EPS = H.EPS
BATCH = 9
NAMES = ("stationarity", "w", "resid")
INF = np.inf

# (m, n): the shapes of tests/test_gpu_batched_bvls.py, wave route then workgroup route (the last: qr_bvls_batched_max_rows(63) x 63)
WAVE_SHAPES = [(1, 1), (2, 2), (3, 2), (8, 7), (16, 7), (16, 15), (64, 15), (64, 31)]
MAX_ROWS_63 = 290
WG_SHAPES = [(65, 31), (40, 32), (100, 33), (256, 40), (130, 63), (63, 63), (MAX_ROWS_63, 63)]
SHAPES = WAVE_SHAPES + WG_SHAPES


def max_rows(n):
    """qr_bvls_batched_max_rows from its byte formula: the largest m <= 512 with 8 ((n + 1) ld(m) + 6 n + 72) <= 160 KiB"""
    if n < 1 or n > 63:
        return 0
    m = 512
    while m >= n and 8 * ((n + 1) * (((m + 29) // 32) * 32 + 2) + 6 * n + 72) > 160 * 1024:
        m -= 1
    return m if m >= n else 0


def gradient(A, b, x, dtype=np.float64):
    """(w, resid) = (A^T (b - A x), ||A x - b||), the residual summed over the columns in ascending order"""
    A, b, x = H.arr(A, dtype), H.arr(b, dtype), H.arr(x, dtype)
    r = b.copy()
    for j in range(A.shape[1]):
        r -= A[:, j] * x[j]
    w = H.arr(np.zeros(A.shape[1]), dtype)
    for j in range(A.shape[1]):
        w[j] = (A[:, j] * r).sum()
    return w, H.norm(r, dtype)


def bvls(A, b, lo=None, hi=None, maxit=0, dtype=np.float64):
    """dict(x, w, state, resid, iter, info) of min ||A x - b|| subject to lo <= x <= hi by the steps of section 8i in `dtype`; x, w, state
    and resid are None where the call writes nothing (info -1 or j + 1)"""
    A, b = H.arr(A, dtype), H.arr(b, dtype)
    m, n = A.shape
    lo = np.full(n, -INF) if lo is None else np.asarray(lo, dtype=np.float64)
    hi = np.full(n, INF) if hi is None else np.asarray(hi, dtype=np.float64)
    maxit = 3 * n if maxit <= 0 else maxit
    nothing = dict(x=None, w=None, state=None, resid=None, iter=None)
    for j in range(n):
        if not (lo[j] <= hi[j]) or lo[j] == INF or hi[j] == -INF:
            return dict(nothing, info=-1)
    # 1. the start
    state = np.array([-1 if lo[j] != -INF else (1 if hi[j] != INF else 0) for j in range(n)])
    x = H.arr([lo[j] if state[j] == -1 else (hi[j] if state[j] == 1 else 0.0) for j in range(n)], dtype)
    lo_t, hi_t = H.arr(lo, dtype), H.arr(hi, dtype)
    it, info, banned = 0, 0, set()
    pend, t, tfrom = False, -1, 0
    test = not np.any(state == 0)
    done = False
    while not done:
        if test:
            # 2. the bound variable that gains most from leaving its bound; ties to the smallest index
            w, _ = gradient(A, b, x, dtype)
            best, bv = -1, 0
            for j in range(n):
                if state[j] == 0 or j in banned or not (lo[j] < hi[j]):
                    continue
                cv = w[j] if state[j] == -1 else -w[j]
                if cv > bv:
                    best, bv = j, cv
            if best < 0:
                break
            t, tfrom, pend = best, state[best], True
            state[best] = 0
        test = True
        while True:
            # 3. one elimination
            if it == maxit:
                info, done = n + 1, True
                break
            it += 1
            free = [j for j in range(n) if state[j] == 0]
            r = b.copy()
            for j in range(n):
                if state[j] != 0:
                    r -= A[:, j] * x[j]
            F, tau = H.qr(A[:, free], dtype)
            nf = len(free)
            for i in range(nf):
                if F[i, i] == 0:
                    return dict(nothing, info=free[i] + 1)
            qtr = H.apply_q(F, tau, r, "T", dtype)
            z = H.solve_r(H.triu(F), qtr[:nf], dtype) if nf else qtr[:0]
            # 4. the variable just freed must move into its box
            if pend:
                pend = False
                zt = z[free.index(t)]
                if (tfrom == -1 and zt <= lo_t[t]) or (tfrom == 1 and zt >= hi_t[t]):
                    state[t] = tfrom
                    banned.add(t)
                    break
            # 5. accept
            if all(lo_t[j] <= z[c] and z[c] <= hi_t[j] for c, j in enumerate(free)):
                for c, j in enumerate(free):
                    x[j] = z[c]
                banned = set()
                break
            # 6. the longest step towards z that stays in the box
            k, amin, kb, ks = -1, INF, 0.0, 0
            for c, j in enumerate(free):
                below = z[c] < lo_t[j]
                if not (below or z[c] > hi_t[j]):
                    continue
                bnd = lo_t[j] if below else hi_t[j]
                al = (bnd - x[j]) / (z[c] - x[j])
                if (al <= amin) if k < 0 else (al < amin):
                    k, amin, kb, ks = j, al, bnd, (-1 if below else 1)
            if k >= 0:
                for c, j in enumerate(free):
                    x[j] = x[j] + amin * (z[c] - x[j])
                x[k], state[k] = kb, ks
                for j in free:
                    if state[j] != 0:
                        continue
                    if x[j] <= lo_t[j]:
                        x[j], state[j] = lo_t[j], -1
                    elif x[j] >= hi_t[j]:
                        x[j], state[j] = hi_t[j], 1
    w, resid = gradient(A, b, x, dtype)
    return dict(x=x, w=w, state=state, resid=resid, iter=it, info=info)


def member(m, n, q, seed):
    """one planted member: (A, b, lo, hi, xstar, state)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    if q % 3 == 1:
        A = A * np.logspace(0, -4, n)[None, :]
    lo, hi = -rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
    kind = rng.choice([0, 0, -1, 1], size=n)                  # about half the variables are active
    inf_side = rng.integers(0, 4, size=n)                      # for a free variable: 0 both finite, 1 lo, 2 hi, 3 both infinite
    u = rng.uniform(0.5, 1.5, n)
    xs = rng.uniform(-0.4, 0.4, n)
    norms = np.linalg.norm(A, axis=0)
    ws = np.zeros(n)
    for j in range(n):
        if kind[j] == 0:
            if inf_side[j] in (1, 3):
                lo[j] = -INF
            if inf_side[j] in (2, 3):
                hi[j] = INF
        elif kind[j] == -1:
            xs[j], ws[j] = lo[j], -u[j] * norms[j]
        else:
            xs[j], ws[j] = hi[j], u[j] * norms[j]
    Q, R = np.linalg.qr(A)
    r = Q @ np.linalg.solve(R.T, ws)
    v = rng.standard_normal(m)
    v -= Q @ (Q.T @ v)
    v -= Q @ (Q.T @ v)
    if m > n:
        r = r + v
    b = A @ xs + r
    return A, b, lo, hi, xs, kind


def measures(A, b, x, w, resid, state):
    """(stationarity, w, resid), evaluated in longdouble; w or resid may be None (their measure is 0)"""
    Al, bl, xl = H.arr(A), H.arr(b), H.arr(x)
    rl = bl - H.matmul(Al, xl[:, None])[:, 0]
    gl = H.matmul(Al.T, rl[:, None])[:, 0]
    nb = float(H.norm(bl))
    nrm = float(H.norm(Al)) * float(H.norm(xl)) + nb
    cn = np.array([float(H.norm(Al[:, j])) for j in range(A.shape[1])])
    stat = max([float(abs(gl[j])) / (cn[j] * nrm) for j in range(A.shape[1]) if state[j] == 0], default=0.0)
    werr = 0.0 if w is None else max(float(abs(H.arr(w)[j] - gl[j])) / (cn[j] * nrm) for j in range(A.shape[1]))
    rerr = 0.0 if resid is None else float(abs(H.arr(np.float64(resid)) - H.norm(rl))) / nb
    return stat, werr, rerr


@functools.lru_cache(maxsize=None)
def case(m, n, batch=BATCH, salt=0):
    """`batch` planted members: A (batch, m, n), b (batch, m), lo, hi, xstar (batch, n), state (batch, n), read-only, and per member out64
    (the float64 instance's result), ref (its measures) and the cap"""
    mem = [member(m, n, q, 100000 * m + 1000 * n + 7919 * q + 77777 * salt + 5) for q in range(batch)]
    out = dict(out64=[], ref=[], cap=(m + n) * EPS)
    for A, b, lo, hi, xs, st in mem:
        o = bvls(A, b, lo, hi)
        out["out64"].append(o)
        out["ref"].append(measures(A, b, o["x"], o["w"], o["resid"], o["state"]) if o["x"] is not None else None)
    for key, idx in (("A", 0), ("b", 1), ("lo", 2), ("hi", 3), ("xstar", 4), ("state", 5)):
        out[key] = np.stack([x[idx] for x in mem])
        out[key].setflags(write=False)
    return out
