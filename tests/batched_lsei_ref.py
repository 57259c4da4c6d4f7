"""Inputs, the restatement and the error measures of the batched inequality-constrained least-squares tests (mi355x_qr.h section 8l; helper
module, no fixtures, no GPU).

`lsei` restates the eight steps of the header's section 8l in straight loops on hp_ref's qr, apply_q and solve_r (no LAPACK); every
candidate is the null-space solve of section 8h on the rows of the set.  Its float64 instance is "the same operation in working precision"
that the GPU test measures the kernels against; the kernels take the same decisions in the same order.

A case is (m, n, mg, neq): `batch` planted members min ||A x - b|| subject to G(0:neq) x = h(0:neq), G(neq:mg) x >= h(neq:mg), m >= n,
whose solution x*, multipliers mu* and active set are known exactly, so that no test depends on the path the restatement takes:
    A, G     standard normal from numpy's default_rng(seed); x* uniform in [-1, 1].  Every third member (q % 3 == 1) has the same column
             grading D = logspace(0, -4, n) on A and on G, with x* divided by D
    active   min(floor(min(n, mg - neq) / 2), n - neq) inequality rows, drawn at random, with mu* in [0.5, 1.5]; equality rows carry mu*
             in +-[0.5, 1.5]; every other row has slack in [0.5, 1.5] ||G_i D^-1||
    h        G x* - slack
    b        A x* - Q R^-T G^T mu* + (a vector orthogonal to range A), A = Q R: A^T (A x* - b) = G^T mu*
Strict complementarity and full rank make x*, mu* and the set unique.

Measures per member, all evaluated in longdouble from the returned values (|.| entrywise):
    feasibility  max_i viol_i / (|G_i| |x| + |h_i|), viol_i = |G_i x - h_i| on equality and active rows, max(0, h_i - G_i x) elsewhere   cap (n + 8) eps
    kkt          max_j |A^T (A x - b) - G^T mu|_j / (||a_j|| (||A||_F ||x|| + ||b||) + (|G|^T |mu|)_j)                                  cap (m + n + mg) eps
    resid        |resid - ||A x - b||| / ||b||                                                                                        cap (m + n + mg) eps
    s            max_i |s_i - (G_i x - h_i)| / (|G_i| |x| + |h_i|)                                                                     cap (n + 8) eps
"""
import functools

import numpy as np

import hp_ref as H

EPS = H.EPS
BATCH = 9
NAMES = ("feasibility", "kkt", "resid", "s")
MAX_N = 63
MAX_MG = 64


def max_rows(n, mg):
    """qr_lsei_batched_max_rows from its byte formula: the largest m <= 512 with
    8 ((n + 1) ld(m) + (n + 1) ld(n) + 5 mg + 4 n + 72) <= 160 KiB, ld(r) = 32 floor((r + 29) / 32) + 2; 0 where (n, mg) is not taken"""
    if n < 1 or n > MAX_N or mg < 1 or mg > MAX_MG:
        return 0
    ld = lambda r: ((r + 29) // 32) * 32 + 2
    m = 512
    while m >= 1 and 8 * ((n + 1) * ld(m) + (n + 1) * ld(n) + 5 * mg + 4 * n + 72) > 160 * 1024:
        m -= 1
    return m if m >= 1 else 0


# (m, n, mg, neq): the shapes of tests/test_gpu_batched_lsei.py, wave route then workgroup route
WAVE_SHAPES = [(1, 1, 1, 0), (2, 2, 1, 1), (3, 2, 5, 0), (8, 7, 3, 1), (16, 7, 20, 2), (16, 15, 15, 0), (64, 15, 64, 4), (64, 31, 40, 0)]
MAX_ROWS_63_64 = 226
WG_SHAPES = [(65, 31, 10, 0), (40, 32, 33, 3), (100, 33, 64, 0), (130, 63, 64, 8), (63, 63, 64, 0), (MAX_ROWS_63_64, 63, 64, 0)]
SHAPES = WAVE_SHAPES + WG_SHAPES


def slack_of(G, h, x, dtype=np.float64):
    """s = G x - h, every row's sum over the columns in ascending order starting from -h_i"""
    G, h, x = H.arr(G, dtype), H.arr(h, dtype), H.arr(x, dtype)
    s = -h
    for j in range(G.shape[1]):
        s = s + G[:, j] * x[j]
    return s


def resid_of(A, b, x, dtype=np.float64):
    """||A x - b||, the residual summed over the columns in ascending order"""
    A, b, x = H.arr(A, dtype), H.arr(b, dtype), H.arr(x, dtype)
    r = b.copy()
    for j in range(A.shape[1]):
        r -= A[:, j] * x[j]
    return H.norm(r, dtype)


def candidate(A, b, G, h, S, dtype):
    """(x_S, zeta, info) of min ||A x - b|| subject to G_S x = h_S, the rows in the order of the list S, by steps 1 to 8 of section 8h
    (a plain factorisation of A for an empty S); zeta = -lambda_S: A^T (A x_S - b) = G_S^T zeta.  info: 0, -3 (an exactly zero
    R_c(i,i)) or i + 1 (an exactly zero R_a(i,i))"""
    m, n = A.shape
    p = len(S)
    k = n - p
    if p == 0:
        Fa, ta = H.qr(A, dtype)
        for i in range(n):
            if Fa[i, i] == 0:
                return None, None, i + 1
        t = H.apply_q(Fa, ta, b, "T", dtype)
        return H.solve_r(H.triu(Fa), t[:n], dtype), t[:0], 0
    C, d = G[S], h[S]
    Fc, tc = H.qr(C.T, dtype)
    for i in range(p):
        if Fc[i, i] == 0:
            return None, None, -3
    Rc = H.triu(Fc)
    y1 = H.solve_rt(Rc, d, dtype)
    At = H.apply_q(Fc, tc, A.T, "T", dtype).T
    r = b.copy()
    for i in range(p):
        r -= At[:, i] * y1[i]
    Fa, ta = H.qr(At[:, p:], dtype)
    for i in range(k):
        if Fa[i, i] == 0:
            return None, None, i + 1
    t = H.apply_q(Fa, ta, r, "T", dtype)
    Gt = H.apply_q(Fa, ta, At[:, :p], "T", dtype)
    y2 = H.solve_r(H.triu(Fa), t[:k], dtype) if k else t[:0]
    x = H.apply_q(Fc, tc, np.concatenate([y1, y2]), "N", dtype)
    g = H.arr(np.zeros(p), dtype)
    for row in range(k, m):
        g += Gt[row] * t[row]
    lam = H.solve_r(Rc, g, dtype)
    return x, -lam, 0


def lsei(A, b, G, h, neq, maxit=0, rcond=0.0, dtype=np.float64):
    """dict(x, mu, s, state, resid, iter, info) of min ||A x - b|| subject to G(0:neq) x = h(0:neq), G(neq:) x >= h(neq:) by the steps of
    section 8l in `dtype`; everything but info is None where the call writes nothing (info -2, -3 or i + 1)"""
    A, b, G, h = H.arr(A, dtype), H.arr(b, dtype), H.arr(G, dtype), H.arr(h, dtype)
    m, n = A.shape
    mg = G.shape[0]
    maxit = 3 * mg + 1 if maxit <= 0 else maxit
    rcond = n * EPS if rcond <= 0 else rcond
    nothing = dict(x=None, mu=None, s=None, state=None, resid=None, iter=None)
    zero = H.arr(np.zeros(mg), dtype)
    # 1. the start
    W = list(range(neq))
    it = 1
    x, zeta, info = candidate(A, b, G, h, W, dtype)
    if info:
        return dict(nothing, info=info)
    mu = zero.copy()
    for c, i in enumerate(W):
        mu[i] = zeta[c]
    accepted = (list(W), mu.copy())
    banned = set()
    info = 0
    while True:
        # 2. the outer test: the most violated row outside the set, ties to the smallest index
        s = slack_of(G, h, x, dtype)
        t, worst = -1, 0
        for i in range(neq, mg):
            if i in W or i in banned:
                continue
            if s[i] < worst:
                t, worst = i, s[i]
        if t < 0:
            break
        mu[t] = 0
        pend = True
        back = False
        while not back:
            # 3. the count
            if it == maxit:
                info = n + 1
                break
            it += 1
            # 4. is G_t a combination of the rows of the set?
            pw = len(W)
            Fc, tc = H.qr(G[W].T, dtype) if pw else (H.arr(np.zeros((n, 0)), dtype), [])
            col = H.apply_q(Fc, tc, G[t], "T", dtype) if pw else G[t].copy()
            rho = H.norm(col[pw:], dtype) if pw < n else 0
            if pw == n or rho <= rcond * H.norm(G[t], dtype):
                c = H.solve_r(H.triu(Fc)[:pw, :pw], col[:pw], dtype) if pw else col[:0]
                k, theta = -1, np.inf
                for pos, i in enumerate(W):
                    if i >= neq and c[pos] > 0:
                        q = mu[i] / c[pos]
                        if q < theta:
                            k, theta = i, q
                if k < 0:
                    return dict(nothing, info=-2)
                for pos, i in enumerate(W):
                    mu[i] = mu[i] - theta * c[pos]
                mu[t] = mu[t] + theta
                mu[k] = 0
                W = [i for i in W if i != k and (i < neq or not mu[i] <= 0)]
                for i in range(neq, mg):
                    if i != t and i not in W:
                        mu[i] = 0
                pend = False
                continue
            # 5. the candidate of the set with t
            S = W + [t]
            xc, zeta, ci = candidate(A, b, G, h, S, dtype)
            if ci:
                return dict(nothing, info=ci)
            # 6. the row just taken must come out with a positive multiplier
            if pend:
                pend = False
                if zeta[-1] <= 0:
                    banned.add(t)
                    mu[t] = 0
                    back = True
                    continue
            # 7. accept
            if all(zeta[pos] > 0 for pos, i in enumerate(S) if i >= neq):
                W = sorted(S)
                mu = zero.copy()
                for pos, i in enumerate(S):
                    mu[i] = zeta[pos]
                x = xc
                accepted = (list(W), mu.copy())
                banned = set()
                back = True
                continue
            # 8. the longest step towards zeta that keeps the multipliers of the inequalities non-negative
            k, alpha = -1, np.inf
            for pos, i in enumerate(S):
                if i >= neq and zeta[pos] <= 0:
                    q = mu[i] / (mu[i] - zeta[pos])
                    if q < alpha or (q == alpha and i < k):
                        k, alpha = i, q
            if k < 0:                 # (a NaN in zeta: nothing moves and the count ends the loop)
                continue
            if k == t:
                # (this does not happen in exact arithmetic) nothing moves: the set and mu are the accepted pair's again, t is banned
                W, mu = list(accepted[0]), accepted[1].copy()
                banned.add(t)
                back = True
                continue
            for pos, i in enumerate(S):
                mu[i] = mu[i] + alpha * (zeta[pos] - mu[i])
            mu[k] = 0
            W = [i for i in W if i != k and (i < neq or not mu[i] <= 0)]
            for i in range(neq, mg):
                if i != t and i not in W:
                    mu[i] = 0
        if info:
            break
    W, mu = accepted
    state = np.array([1 if i in W else 0 for i in range(mg)])
    return dict(x=x, mu=mu, s=slack_of(G, h, x, dtype), state=state, resid=resid_of(A, b, x, dtype), iter=it, info=info)


def member(m, n, mg, neq, q, seed):
    """one planted member: (A, b, G, h, xstar, mustar, state)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n))
    G = rng.standard_normal((mg, n))
    xs = rng.uniform(-1.0, 1.0, n)
    D = np.logspace(0, -4, n) if q % 3 == 1 else np.ones(n)
    A, G, xs = A * D[None, :], G * D[None, :], xs / D
    na = min(min(n, mg - neq) // 2, n - neq)
    state = np.zeros(mg, dtype=np.int64)
    state[:neq] = 1
    state[neq + rng.permutation(mg - neq)[:na]] = 1
    mus = rng.uniform(0.5, 1.5, mg) * state
    mus[:neq] *= rng.choice([-1.0, 1.0], size=neq)
    slack = rng.uniform(0.5, 1.5, mg) * np.linalg.norm(G / D[None, :], axis=1) * (1 - state)
    h = G @ xs - slack
    Q, R = np.linalg.qr(A)
    r = Q @ np.linalg.solve(R.T, G.T @ mus)
    v = rng.standard_normal(m)
    v -= Q @ (Q.T @ v)
    v -= Q @ (Q.T @ v)
    if m > n:
        r = r - v
    b = A @ xs - r
    return A, b, G, h, xs, mus, state


def measures(A, b, G, h, x, mu, s, resid, state):
    """(feasibility, kkt, resid, s), evaluated in longdouble; mu, s or resid may be None (their measure is 0)"""
    Al, bl, Gl, hl, xl = H.arr(A), H.arr(b), H.arr(G), H.arr(h), H.arr(x)
    rl = H.matmul(Al, xl[:, None])[:, 0] - bl
    sl = H.matmul(Gl, xl[:, None])[:, 0] - hl
    scale = [float((abs(Gl[i]) * abs(xl)).sum() + abs(hl[i])) for i in range(G.shape[0])]
    feas = 0.0
    for i in range(G.shape[0]):
        viol = abs(sl[i]) if state[i] else max(-sl[i], 0 * sl[i])
        if scale[i] != 0:
            feas = max(feas, float(viol) / scale[i])
    kkt = 0.0
    if mu is not None:
        ml = H.arr(mu)
        gl = H.matmul(Al.T, rl[:, None])[:, 0] - H.matmul(Gl.T, ml[:, None])[:, 0]
        nrm = float(H.norm(Al)) * float(H.norm(xl)) + float(H.norm(bl))
        for j in range(A.shape[1]):
            den = float(H.norm(Al[:, j])) * nrm + float((abs(Gl[:, j]) * abs(ml)).sum())
            kkt = max(kkt, float(abs(gl[j])) / den)
    rerr = 0.0 if resid is None else float(abs(H.arr(np.float64(resid)) - H.norm(rl))) / float(H.norm(bl))
    serr = 0.0
    if s is not None:
        for i in range(G.shape[0]):
            if scale[i] != 0:
                serr = max(serr, float(abs(H.arr(s)[i] - sl[i])) / scale[i])
    return feas, kkt, rerr, serr


def caps(m, n, mg):
    return ((n + 8) * EPS, (m + n + mg) * EPS, (m + n + mg) * EPS, (n + 8) * EPS)


@functools.lru_cache(maxsize=None)
def case(m, n, mg, neq, batch=BATCH, salt=0):
    """`batch` planted members: A (batch, m, n), b (batch, m), G (batch, mg, n), h (batch, mg), xstar, mustar, state, read-only, and per
    member out64 (the float64 instance's result), ref (its measures) and the caps"""
    mem = [member(m, n, mg, neq, q, 100000 * m + 1000 * n + 10 * mg + neq + 7919 * q + 77777 * salt + 11) for q in range(batch)]
    out = dict(out64=[], ref=[], caps=caps(m, n, mg))
    for A, b, G, h, xs, mus, st in mem:
        o = lsei(A, b, G, h, neq)
        out["out64"].append(o)
        out["ref"].append(measures(A, b, G, h, o["x"], o["mu"], o["s"], o["resid"], o["state"]) if o["x"] is not None else None)
    for key, idx in (("A", 0), ("b", 1), ("G", 2), ("h", 3), ("xstar", 4), ("mustar", 5), ("state", 6)):
        out[key] = np.stack([x[idx] for x in mem])
        out[key].setflags(write=False)
    return out


# the two specials of the header: rows (G, h), no equalities, with A = I and b = 0 (x is the point of the set nearest the origin)
DEPENDENT_FEASIBLE = (np.array([[1.0, 0.0], [2.0, 0.0], [0.0, 1.0], [0.0, -1.0]]), np.array([1.0, 1.0, 0.5, -0.5]))
INFEASIBLE = (np.array([[1.0, 0.0], [-1.0, 0.0]]), np.array([1.0, 0.0]))
