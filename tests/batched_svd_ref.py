"""A numpy restatement of the batched SVD's steps 2 to 5 (mi355x_qr.h section 8c; kernel: csrc/qr_batched_svd.hip), and the shapes and
input classes its tests share (test_batched_svd_ref.py without a GPU, test_gpu_batched_svd.py with one).

jsvd_ref(R, jpvt) -> (S, V, W, rank, sweeps): from the triangle and permutation of a column-pivoted QR, A P = Q R,

  2. the rank cut r = the leading run of |R(i,i)| > sqrt(n) eps |R(0,0)|, rows r.. of R dropped,
  3. one-sided Jacobi on G = (R with rows r.. zeroed)^T in the round-robin circle ordering over the columns (circle_pairs: the
     ordering of qr_jsvd_round_pairs with blocks of one column), the rotation of the smaller angle, the pair skipped where a or b is 0,
     where |c| <= tol sqrt(a) sqrt(b) (tol = sqrt(n) eps) or where it is not live (a > eps^2 b and b > eps^2 a); W receives the rotations;
     the first sweep that rotates nothing ends the iteration and is counted; MAX_SWEEPS is the limit,
  4. S = the column norms, sorted descending and stably; the live columns of V-hat = the normalised columns of G; V = P V-hat,
  5. where r < n the columns of V for S = 0 are the trailing columns of the Q of a Householder QR of the live block.

Then A = (Q [W; 0]) diag(S) V^T with W's columns in the sorted order.  The sums are numpy's, not the kernel's lane-group sums: values
agree to rounding, sweep counts to the odd borderline pair.
"""
import numpy as np

import hp_ref as H

EPS = np.finfo(np.float64).eps
MAX_SWEEPS = 30                           # QR_JSVD_MAX_SWEEPS

# the smallest shapes that reach every route and edge of the kernel (the table of the section's tests)
SHAPES = [(1, 1), (2, 2), (3, 3), (5, 3), (8, 8), (33, 17), (64, 32), (65, 33), (100, 33), (64, 64), (256, 64), (512, 32), (290, 64)]
# exact ranks: (m, n) -> r
RANKS = {(64, 32): 5, (256, 64): 10, (100, 33): 1, (3, 3): 2, (64, 64): 63}
BATCH = 5                                 # no multiple of four


def circle_pairs(n, rd):
    """the disjoint pairs (p, q), p < q, of round rd over n columns; n odd: n rounds, n even: n - 1 rounds, n // 2 pairs each"""
    if n < 2:
        return []
    N = n if n & 1 else n - 1
    out = [] if n & 1 else [(rd, n - 1)]
    for k in range(1, (N - 1) // 2 + 1):
        a, b = (rd + k) % N, (rd - k + N) % N
        out.append((min(a, b), max(a, b)))
    return out


def rounds(n):
    return 0 if n < 2 else (n if n & 1 else n - 1)


def rank_cut(R):
    n = R.shape[1]
    d = np.abs(np.diag(R))
    if d[0] == 0.0:
        return 0
    small = np.flatnonzero(~(d > np.sqrt(n) * EPS * d[0]))
    return int(small[0]) if small.size else n


def jsvd_ref(R, jpvt, want_w=True):
    R = np.triu(np.asarray(R, dtype=np.float64))
    n = R.shape[1]
    R = R[:n]
    r = rank_cut(R)
    G = np.zeros((n, n))
    G[:, :r] = R[:r].T
    W = np.eye(n)
    tol = np.sqrt(n) * EPS
    sweeps, done = 0, False
    while not done and sweeps < MAX_SWEEPS:
        rotated = False
        for rd in range(rounds(n)):
            for p, q in circle_pairs(n, rd):
                if q >= r:                                   # (an exact zero column: a or b is 0)
                    continue
                gp, gq = G[:, p].copy(), G[:, q].copy()
                a, b, c = float(gp @ gp), float(gq @ gq), float(gp @ gq)
                if a == 0.0 or b == 0.0 or not (a > EPS * EPS * b and b > EPS * EPS * a):
                    continue
                if abs(c) <= tol * np.sqrt(a) * np.sqrt(b):
                    continue
                zeta = (b - a) / (2.0 * c)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = cs * t
                G[:, p], G[:, q] = cs * gp - sn * gq, sn * gp + cs * gq
                if want_w:
                    wp, wq = W[:, p].copy(), W[:, q].copy()
                    W[:, p], W[:, q] = cs * wp - sn * wq, sn * wp + cs * wq
                rotated = True
        sweeps += 1
        done = not rotated
    sig = np.sqrt((G * G).sum(axis=0))
    order = np.argsort(-sig, kind="stable")
    S = sig[order]
    rank = int(np.count_nonzero(S))
    Vh = np.zeros((n, n))
    live = sig > 0
    Vh[:, live] = G[:, live] / sig[live]
    if r < n:
        Qf = np.linalg.qr(Vh[:, :r], mode="complete")[0] if r else np.eye(n)
        Vh[:, r:] = Qf[:, r:]
    V = np.empty((n, n))
    V[np.asarray(jpvt)] = Vh[:, order]
    return S, V, W[:, order], rank, sweeps


def dlaqp2(A):
    """LAPACK dlaqp2 with every column free: (F, tau, jpvt), F in dgeqr2's layout, jpvt 0-based"""
    F = np.array(A, dtype=np.float64)
    m, n = F.shape
    jpvt, tau = np.arange(n), np.zeros(n)
    vn1 = np.sqrt((F * F).sum(axis=0))
    vn2 = vn1.copy()
    for j in range(n):
        p = j + int(np.argmax(vn1[j:]))
        if p != j:
            F[:, [j, p]] = F[:, [p, j]]
            jpvt[[j, p]] = jpvt[[p, j]]
            vn1[p], vn2[p] = vn1[j], vn2[j]
        x = F[j + 1:, j]
        ssq = float(x @ x)
        e = H.column_scale(x, ssq)              # (the column step's guard: a rounding-sized column of tiny data is scaled before it is squared)
        xs = np.ldexp(x, -e)
        xnorm = float(np.ldexp(np.sqrt(float(xs @ xs)), e)) if e else np.sqrt(ssq)
        if xnorm != 0.0:
            alpha = F[j, j]
            beta = -np.copysign(np.hypot(alpha, xnorm), alpha)
            tau[j] = (beta - alpha) / beta
            v = np.concatenate(([1.0], x / (alpha - beta)))
            F[j:, j + 1:] -= tau[j] * np.outer(v, v @ F[j:, j + 1:])
            F[j, j] = beta
            F[j + 1:, j] = v[1:]
        for c in range(j + 1, n):
            if vn1[c] == 0.0:
                continue
            t = abs(F[j, c]) / vn1[c]
            temp = max(0.0, 1.0 - t * t)
            if temp * (vn1[c] / vn2[c]) ** 2 <= np.sqrt(EPS):
                vn1[c] = vn2[c] = np.sqrt(float(F[j + 1:, c] @ F[j + 1:, c]))
            else:
                vn1[c] *= np.sqrt(temp)
    return F, tau, jpvt


def form_q(F, tau):
    """the thin m x n Q of dgeqr2's layout"""
    m, n = F.shape
    Q = np.eye(m, n)
    for j in range(n - 1, -1, -1):
        v = np.concatenate(([1.0], F[j + 1:, j]))
        Q[j:, :] -= tau[j] * np.outer(v, v @ Q[j:, :])
    return Q


# ---- input classes: every one returns (A (batch, m, n), true ranks (batch,) or None) ----
def _ortho(rng, m, k):
    return np.linalg.qr(rng.standard_normal((m, k)))[0]


def with_cond(rng, m, n, kappa):
    s = kappa ** (-np.arange(n) / max(n - 1, 1))
    return (_ortho(rng, m, n) * s) @ _ortho(rng, n, n).T


def with_rank(rng, m, n, r):
    return rng.standard_normal((m, r)) @ rng.standard_normal((r, n))


def zero_and_duplicate(rng, m, n):
    A = rng.standard_normal((m, n))
    if n >= 3:
        A[:, 1] = 0.0
        A[:, n - 1] = A[:, 0]
    elif n == 2:
        A[:, 1] = A[:, 0]
    return A


def true_rank_zero_dup(m, n):
    return n - 2 if n >= 3 else 1


KINDS = ("gaussian", "cond1e6", "cond1e12", "rank", "zerodup", "zero", "identity", "mixed")


def make_batch(kind, m, n, batch=BATCH):
    """the batch of one input class at one shape, and the true rank of every matrix where the class fixes it (else None)"""
    rng = np.random.default_rng(1000 * m + 10 * n + KINDS.index(kind))
    if kind == "gaussian":
        return rng.standard_normal((batch, m, n)), None
    if kind in ("cond1e6", "cond1e12"):
        return np.stack([with_cond(rng, m, n, float(kind[4:])) for _ in range(batch)]), None
    if kind == "rank":
        r = RANKS[(m, n)]
        return np.stack([with_rank(rng, m, n, r) for _ in range(batch)]), np.full(batch, r)
    if kind == "zerodup":
        return np.stack([zero_and_duplicate(rng, m, n) for _ in range(batch)]), np.full(batch, true_rank_zero_dup(m, n))
    if kind == "zero":
        return np.zeros((batch, m, n)), np.zeros(batch, dtype=int)
    if kind == "identity":
        return np.stack([np.eye(m, n)] * batch), np.full(batch, n)
    r = RANKS.get((m, n), max(n // 2, 1))                    # mixed: several classes side by side
    mats = [rng.standard_normal((m, n)), with_rank(rng, m, n, r), np.zeros((m, n)), with_cond(rng, m, n, 1e12), zero_and_duplicate(rng, m, n),
            np.eye(m, n), with_cond(rng, m, n, 1e6)]
    return np.stack([mats[i % len(mats)] for i in range(batch)]), None


def cases():
    """(kind, m, n) of every test case: every class at every shape, the exact ranks at their own shapes"""
    out = []
    for kind in KINDS:
        for (m, n) in SHAPES:
            if kind == "rank" and (m, n) not in RANKS:
                continue
            out.append((kind, m, n))
    return out


def errors(A, U, S, V, sweeps):
    """the four measured errors of one matrix and the unit s n eps they are bounded in: (rec, sig, ov, ou, unit)"""
    m, n = A.shape
    unit = sweeps * n * EPS
    an = np.linalg.norm(A)
    rec = np.linalg.norm(A - (U * S) @ V.T) / (an if an > 0 else 1.0)
    sn = np.linalg.svd(A, compute_uv=False)
    sig = np.max(np.abs(S - sn)) / (sn[0] if sn[0] > 0 else 1.0)
    ov = np.linalg.norm(V.T @ V - np.eye(n))
    ou = np.linalg.norm(U.T @ U - np.eye(n))
    return rec, sig, ov, ou, unit


def check_bounds(A, U, S, V, sweeps):
    """the section's bounds on one matrix; returns the four errors as fractions of their bounds"""
    n = A.shape[1]
    rec, sig, ov, ou, unit = errors(A, U, S, V, sweeps)
    extra = (n + 8) * EPS
    fr = (rec / (unit + extra), sig / (unit + extra), ov / (4 * unit), ou / (4 * unit + extra))
    assert rec <= unit + extra, ("reconstruction", rec / EPS, (unit + extra) / EPS)
    assert sig <= unit + extra, ("sigma", sig / EPS, (unit + extra) / EPS)
    assert ov <= 4 * unit, ("V orthogonality", ov / EPS, 4 * unit / EPS)
    assert ou <= 4 * unit + extra, ("U orthogonality", ou / EPS, (4 * unit + extra) / EPS)
    assert np.all(S >= 0) and np.all(np.diff(S) <= 0)
    return fr
