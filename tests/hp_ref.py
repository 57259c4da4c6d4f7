"""A plain extended-precision reference for the factor and solve paths (helper module, no fixtures, no GPU).

Everything is written as straight loops over columns in numpy, without LAPACK, and is parameterised by dtype: the `longdouble`
instance (64-bit significand) is the reference, the `float64` instance of the very same code is "the same operation in working precision"
that the GPU tests measure the kernels' errors against.  The Householder convention is LAPACK's dgeqr2 / dlarfg (beta = -sign(alpha)
||x||, tau = (beta - alpha) / beta, v = x / (alpha - beta) with a unit head, an exactly zero tail gives tau = 0) without dlarfg's
rescaling of tiny vectors.  Sums of squares are plain `(x * x).sum()`: for a power of two s every function here is exactly
homogeneous while nothing leaves the normal range, which tests/test_hp_ref.py asserts bitwise.

The last block restates single kernels rather than entry points, for the launch-layer tests (test_gpu_update_kernels.py,
test_gpu_svd_kernels.py): tp_panel and tp_apply in the convention of csrc/qr_update.hip, jacobi_pair after jsvd_pair_kernel.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).nmant < 63:          # a platform whose long double is a double: 40 decimal digits through mpmath objects instead
    import mpmath

    mpmath.mp.dps = 40
    LD = np.dtype(object)
    _lift = np.frompyfunc(mpmath.mpf, 1, 1)
    _sqrt = np.frompyfunc(mpmath.sqrt, 1, 1)
    EPS_LD = 10.0 ** -39
else:
    assert np.finfo(LD).nmant >= 63
    _lift, _sqrt = None, np.sqrt
    EPS_LD = float(np.finfo(LD).eps)
EPS = float(np.finfo(np.float64).eps)


def arr(A, dtype=LD):
    """a fresh array of A's values in `dtype` (exact for float64 input)"""
    A = np.asarray(A)
    if dtype is LD and _lift is not None:
        return _lift(np.asarray(A, dtype=np.float64)).astype(object)
    return np.array(A, dtype=dtype)


def _root(x, dtype):
    return _sqrt(x) if (dtype is LD and _lift is not None) else np.sqrt(x)


def norm(x, dtype=LD):
    """Frobenius norm, accumulated in `dtype`"""
    x = arr(x, dtype)
    return _root((x * x).sum(), dtype)


SSQ_WINDOW = 900


def ssq_is_plain(ssq):
    """qb_ssq_plain of csrc/qr_batched_dev.h: the plain sum of squares lies within 2^-+SSQ_WINDOW, so its square root is the norm"""
    return np.ldexp(1.0, -SSQ_WINDOW) <= ssq <= np.ldexp(1.0, SSQ_WINDOW)


def column_scale(x, ssq):
    """the exponent e by which the float64 column x, of plain sum of squares ssq, is scaled before it is squared (x 2^-e), as the
    Householder column step of the batched kernels does (qb_wave_nrm, qb_wg_col of csrc/qr_batched_dev.h): 0 while ssq lies inside the
    window, or where the largest |x_i| is 0 or no finite number; else the exponent that brings the largest |x_i| into [1, 2)"""
    if ssq_is_plain(ssq):
        return 0
    xmax = float(np.max(np.abs(x), initial=0.0))
    if xmax == 0 or not np.isfinite(xmax):
        return 0
    return int(np.frexp(xmax)[1]) - 1


def _house(x, dtype):
    """dlarfg on x (modified in place: x[0] <- beta, x[1:] <- v's tail); returns tau.  In float64 a tail whose plain sum of squares
    leaves 2^-+SSQ_WINDOW is scaled by a power of two first (column_scale): exact, so the homogeneity holds bit for bit as before
    wherever no square leaves the normal range, and a rounding-sized column of data near 1e-145 keeps a reflector that is one"""
    alpha = x[0]
    ssq = (x[1:] * x[1:]).sum() if x.size > 1 else 0
    if ssq == 0 and not (dtype is np.float64 and x.size > 1 and np.any(x[1:] != 0)):
        return alpha * 0
    e = column_scale(x[1:], ssq) if dtype is np.float64 else 0
    if e:
        xs, al = np.ldexp(x[1:], -e), np.ldexp(alpha, -e)
        nrm = np.ldexp(_root(al * al + (xs * xs).sum(), dtype), e)
    else:
        nrm = _root(alpha * alpha + ssq, dtype)
    beta = -nrm if alpha >= 0 else nrm
    x[1:] = x[1:] / (alpha - beta)
    x[0] = beta
    return (beta - alpha) / beta


def _reflect(v_tail, tau, C):
    """C <- (I - tau v v^T) C with v = [1; v_tail], in place"""
    if tau == 0 or C.shape[1] == 0:
        return
    w = C[0] + (v_tail[:, None] * C[1:]).sum(axis=0)
    C[0] -= tau * w
    C[1:] -= tau * v_tail[:, None] * w[None, :]


def qr(A, dtype=LD):
    """dgeqr2: (F, tau) with R in F's upper triangle and the tails of v below the diagonal"""
    F = arr(A, dtype)
    m, n = F.shape
    k = min(m, n)
    tau = arr(np.zeros(k), dtype)
    for j in range(k):
        tau[j] = _house(F[j:, j], dtype)
        _reflect(F[j + 1:, j], tau[j], F[j:, j + 1:])
    return F, tau


def apply_q(F, tau, C, trans, dtype=LD):
    """Q^T C (trans 'T') or Q C ('N') for the m x m Q of (F, tau); C has m rows"""
    F, C = arr(F, dtype), arr(C, dtype)
    if C.ndim == 1:
        return apply_q(F, tau, C[:, None], trans, dtype)[:, 0]
    tau = arr(tau, dtype)
    k = len(tau)
    for j in (range(k) if trans == "T" else range(k - 1, -1, -1)):
        _reflect(F[j + 1:, j], tau[j], C[j:])
    return C


def form_q(F, tau, dtype=LD):
    """the explicit thin Q (m x n)"""
    m, n = np.shape(F)
    return apply_q(F, tau, np.eye(m, min(m, n)), "N", dtype)


def triu(F):
    n = min(np.shape(F))
    return np.triu(np.asarray(F)[:n, :n])


def solve_r(R, B, dtype=LD):
    """upper back substitution X = R^-1 B, column-oriented as dtrsm's"""
    R, X = arr(R, dtype), arr(B, dtype)
    vec = X.ndim == 1
    X = X[:, None] if vec else X
    for i in range(R.shape[0] - 1, -1, -1):
        X[i] = X[i] / R[i, i]
        X[:i] -= R[:i, i][:, None] * X[i][None, :]
    return X[:, 0] if vec else X


def solve_rt(R, B, dtype=LD):
    """forward substitution X = R^-T B"""
    R, X = arr(R, dtype), arr(B, dtype)
    vec = X.ndim == 1
    X = X[:, None] if vec else X
    n = R.shape[0]
    for i in range(n):
        X[i] = X[i] / R[i, i]
        X[i + 1:] -= R[i, i + 1:][:, None] * X[i][None, :]
    return X[:, 0] if vec else X


def lstsq(A, B, dtype=LD):
    """min ||A X - B|| for a full-rank tall A: (X, residual norms per column)"""
    F, tau = qr(A, dtype)
    n = F.shape[1]
    B = arr(B, dtype)
    vec = B.ndim == 1
    Y = apply_q(F, tau, B[:, None] if vec else B, "T", dtype)
    X = solve_r(triu(F), Y[:n], dtype)
    res = _root((Y[n:] * Y[n:]).sum(axis=0), dtype)
    return (X[:, 0], res[0]) if vec else (X, res)


def minnorm(A, B, dtype=LD):
    """the minimum-norm solution of A X = B for a full-rank wide A (m <= n): X = Q [R^-T B ; 0] with A^T = Q R"""
    A = arr(A, dtype)
    m, n = A.shape
    F, tau = qr(A.T, dtype)
    B = arr(B, dtype)
    vec = B.ndim == 1
    Y = arr(np.zeros((n, 1 if vec else B.shape[1])), dtype)
    Y[:m] = solve_rt(triu(F), B[:, None] if vec else B, dtype)
    X = apply_q(F, tau, Y, "N", dtype)
    return X[:, 0] if vec else X


def append_rows(R, B, dtype=LD):
    """(F, tau) of the QR of [R ; B]: R' in the upper triangle (the row-append update's result)"""
    return qr(np.vstack([arr(triu(R), dtype), arr(B, dtype)]), dtype)


def remove_rows(A, keep, dtype=LD):
    """R of the rows of A that survive a removal (boolean mask or index list `keep`)"""
    return triu(qr(arr(A, dtype)[keep], dtype)[0])


def qrp(A, dtype=LD):
    """greedy column-pivoted QR with dlaqp2's rule: (F, tau, jpvt 0-based).  The partial norms are downdated by
    vn1 *= sqrt(max(0, 1 - (|F(j,c)| / vn1)^2)) and recomputed when that times (vn1 / vn2)^2 is at most sqrt(eps of float64); the
    first maximum wins a tie."""
    F = arr(A, dtype)
    m, n = F.shape
    k = min(m, n)
    jpvt, tau = np.arange(n), arr(np.zeros(k), dtype)
    vn1 = _root((F * F).sum(axis=0), dtype)
    vn2 = vn1.copy()
    tol3z = np.sqrt(EPS)
    for j in range(k):
        p = j + int(np.argmax(vn1[j:]))
        if p != j:
            F[:, [j, p]] = F[:, [p, j]]
            jpvt[[j, p]] = jpvt[[p, j]]
            vn1[p], vn2[p] = vn1[j], vn2[j]
        tau[j] = _house(F[j:, j], dtype)
        _reflect(F[j + 1:, j], tau[j], F[j:, j + 1:])
        for c in range(j + 1, n):
            if vn1[c] == 0:
                continue
            t = abs(F[j, c]) / vn1[c]
            temp = max(t * 0, 1 - t * t)
            r = vn1[c] / vn2[c]
            if temp * r * r <= tol3z:
                x = F[j + 1:, c]
                vn1[c] = vn2[c] = _root((x * x).sum(), dtype) if x.size else t * 0
            else:
                vn1[c] = vn1[c] * _root(temp, dtype)
    return F, tau, jpvt


# ---- error measures, all evaluated in extended precision (inputs of any dtype) ------------------------------------------------------
def trsm_backward_errors(R, X, B, trans=False):
    """||op(R) x - b|| / (||R|| ||x|| + ||b||) of every column"""
    R, X, B = arr(triu(R)), arr(X), arr(B)
    X, B = (X[:, None], B[:, None]) if X.ndim == 1 else (X, B)
    M = R.T if trans else R
    nR = norm(R)
    out = np.zeros(X.shape[1])
    for j in range(X.shape[1]):
        r = (M * X[:, j][None, :]).sum(axis=1) - B[:, j]
        den = nR * norm(X[:, j]) + norm(B[:, j])
        out[j] = float(norm(r) / den) if den != 0 else 0.0
    return out


def trsm_backward_error(R, X, B, trans=False):
    """the worst column's"""
    return float(trsm_backward_errors(R, X, B, trans).max())


def matmul(A, B):
    """A @ B in extended precision by outer products (no BLAS)"""
    A, B = arr(A), arr(B)
    out = arr(np.zeros((A.shape[0], B.shape[1])))
    for k in range(A.shape[1]):
        out += A[:, k][:, None] * B[k][None, :]
    return out


def apply_error(ref, out, C):
    """||ref - out|| / ||C||"""
    return float(norm(arr(ref) - arr(out)) / norm(C))


def factor_errors(A, Q, R):
    """(||A - Q R|| / ||A||, ||Q^T Q - I||) for a thin Q"""
    A, Q, R = arr(A), arr(Q), arr(R)
    n = Q.shape[1]
    return float(norm(A - matmul(Q, R)) / norm(A)), float(norm(matmul(Q.T, Q) - arr(np.eye(n))))


def normal_equations_residual(A, X, B):
    """||A^T (A x - b)|| / (||A||^2 ||x|| + ||A|| ||b||), the worst column"""
    A, X, B = arr(A), arr(X), arr(B)
    X, B = (X[:, None], B[:, None]) if X.ndim == 1 else (X, B)
    g = matmul(A.T, matmul(A, X) - B)
    nA = norm(A)
    return max(float(norm(g[:, j]) / (nA * nA * norm(X[:, j]) + nA * norm(B[:, j]))) for j in range(X.shape[1]))


# ---- the launch layer of the row updates and of the Jacobi SVD (csrc/qr_update.hip, csrc/qr_svd.hip) ----------------------------------
def _signs(p, p_add, dtype):
    """the diagonal of S: +1 for the block's first p_add rows, -1 for the others"""
    s = arr(np.ones(p), dtype)
    s[p_add:] = -s[p_add:]
    return s


def tp_panel(R, B, p_add=None, dtype=LD):
    """(R', V, T) of the panel [R (w x w upper triangle) ; B (p x w)] under the signs S = diag(+1 (p_add times), -1), the convention at
    the top of csrc/qr_update.hip: reflector j is I - tau_j u_j u_j^T Phi with u_j = [e_j ; V(:, j)], Phi = diag(I, S);
    d = alpha^2 + b^T S b, beta = -sign(alpha) sqrt(d), tau = (beta - alpha) / beta, v = b / (alpha - beta); every product over the
    block's rows is weighted by S; T by dlarft, forward columnwise, with those weighted dots.  p_add = p (the default) is the unsigned
    instance.  An exactly zero column of B gives tau = 0 and changes nothing; d <= 0 raises ArithmeticError with the column in args[1]."""
    Rn, V = arr(triu(R), dtype), arr(B, dtype)
    p, w = V.shape
    p_add = p if p_add is None else p_add
    s = _signs(p, p_add, dtype)
    T = arr(np.zeros((w, w)), dtype)
    for j in range(w):
        b = V[:, j]
        if not np.any(b != 0):
            continue
        alpha = Rn[j, j]
        d = alpha * alpha + (s * b * b).sum()
        if not d > 0:
            raise ArithmeticError("no positive-definite triangle is left", j)
        beta = -_root(d, dtype) if alpha >= 0 else _root(d, dtype)
        tau = (beta - alpha) / beta
        V[:, j] = b / (alpha - beta)
        Rn[j, j] = beta
        sv = s * V[:, j]
        for c in range(j + 1, w):
            tw = tau * (Rn[j, c] + (sv * V[:, c]).sum())
            Rn[j, c] -= tw
            V[:, c] -= tw * V[:, j]
        dots = [(sv * V[:, l]).sum() for l in range(j)]
        for i in range(j):
            T[i, j] = -tau * sum(T[i, l] * dots[l] for l in range(i, j))
        T[j, j] = tau
    return Rn, V, T


def tp_apply(V, T, C1, C2, p_add=None, trans=1, dtype=LD):
    """(C1 - W, C2 - V W) with W = op(T) (C1 + V^T S C2): V p x w, T w x w (only its upper triangle is read), C1 w x ncols, C2 p x ncols.
    op(T) = T^T for trans != 0 and whenever the call is signed (p_add < p), else T."""
    V, C1, C2 = arr(V, dtype), arr(C1, dtype), arr(C2, dtype)
    p, w = V.shape
    p_add = p if p_add is None else p_add
    s = _signs(p, p_add, dtype)
    Tu = arr(np.zeros((w, w)), dtype)
    for j in range(w):
        Tu[:j + 1, j] = arr(np.asarray(T)[:j + 1, j], dtype)
    op = Tu.T if (trans or p_add < p) else Tu
    W0 = C1.copy()
    for i in range(p):
        W0 += (s[i] * V[i])[:, None] * C2[i][None, :]
    W = W0 * 0
    for k in range(w):
        W += op[:, k][:, None] * W0[k][None, :]
    C2n = C2.copy()
    for k in range(w):
        C2n -= V[:, k][:, None] * W[k][None, :]
    return C1 - W, C2n


JS_SLOTS = 64                 # a block pair of csrc/qr_svd.hip: two blocks of 32 columns
JS_INNER_MAX = 16


def js_live(a, b):
    """the columns of squared norms a, b take part in the measure and are rotated: neither is negligible beside the other"""
    e2 = EPS * EPS
    return a > 0 and b > 0 and a > e2 * b and b > e2 * a


def js_inner_pair(st, k):
    """the k-th of the 32 disjoint index pairs (i < j) of step st (0 .. 62) of the round-robin over 64 indices: 63 stays, the others turn"""
    m = JS_SLOTS - 1
    a, b = (st, m) if k == 0 else ((st + k) % m, (st - k + m) % m)
    return min(a, b), max(a, b)


def gram_measure(S, dtype=LD):
    """max over the live pairs i < j of |s_ij| / (sqrt(s_ii) sqrt(s_jj))"""
    k = S.shape[0]
    rt = _root(arr([S[i, i] if S[i, i] > 0 else 0 for i in range(k)], dtype), dtype)
    v = S[0, 0] * 0
    for j in range(k):
        for i in range(j):
            if js_live(S[i, i], S[j, j]):
                v = max(v, abs(S[i, j]) / (rt[i] * rt[j]))
    return v


def gram(G, dtype=LD):
    G = arr(G, dtype)
    S = arr(np.zeros((G.shape[1], G.shape[1])), dtype)
    for i in range(G.shape[0]):
        S += G[i][:, None] * G[i][None, :]
    return S


def pair_measure(G, dtype=LD):
    """the measure of the columns of G (the Gram matrix formed in `dtype`)"""
    return gram_measure(gram(G, dtype), dtype)


def jacobi_pair(G, tol, dtype=LD, wp=None):
    """(measure, G J, J) of one block pair, steps 1-4 of jsvd_pair_kernel on the pair's k <= 64 columns (the first wp of them are the first
    block's and sit in slots 0 .., the others in slots 32 ..; default: min(k, 32)): the Gram matrix S; the measure over the live pairs,
    at or below tol nothing happens (J = I); else cyclic sweeps (at most 16) of 63 round-robin steps of 32 disjoint rotations each on S,
    the angles of a step taken from S as the step found it, the root of smaller modulus of tan^2 + 2 zeta tan - 1 = 0, a pair rotated
    only when live and above tol; J <- J R with cos written as 1 - s^2 / (1 + c); a sweep that leaves the measure at or below tol is
    the last."""
    G = arr(G, dtype)
    k = G.shape[1]
    wp = min(k, JS_SLOTS // 2) if wp is None else wp
    col = {**{i: i for i in range(wp)}, **{JS_SLOTS // 2 + i: wp + i for i in range(k - wp)}}         # slot -> column
    S = gram(G, dtype)
    J = arr(np.eye(k), dtype)
    off = gram_measure(S, dtype)
    if not off > tol:
        return off, G, J
    one = S[0, 0] * 0 + 1
    for _ in range(JS_INNER_MAX):
        for st in range(JS_SLOTS - 1):
            rots = []
            for q in range(JS_SLOTS // 2):
                si, sj = js_inner_pair(st, q)
                if si not in col or sj not in col:
                    continue
                i, j = col[si], col[sj]
                a, b, g = S[i, i], S[j, j], S[i, j]
                if js_live(a, b) and abs(g) > tol * (_root(a, dtype) * _root(b, dtype)):
                    zeta = (b - a) / (2 * g)
                    tn = (one if zeta >= 0 else -one) / (abs(zeta) + _root(1 + zeta * zeta, dtype))
                    c = 1 / _root(1 + tn * tn, dtype)
                    s = c * tn
                    rots.append((i, j, c, s, s * s / (1 + c)))
            for i, j, c, s, h in rots:
                ci, cj = S[:, i].copy(), S[:, j].copy()
                S[:, i], S[:, j] = c * ci - s * cj, s * ci + c * cj
                ri, rj = S[i].copy(), S[j].copy()
                S[i], S[j] = c * ri - s * rj, s * ri + c * rj
                S[i, j] = S[j, i] = S[i, j] * 0
                ji, jj = J[:, i].copy(), J[:, j].copy()
                J[:, i], J[:, j] = ji - (h * ji + s * jj), jj + (s * ji - h * jj)
        if not gram_measure(S, dtype) > tol:
            break
    GJ = G * 0
    for l in range(k):
        GJ += G[:, l][:, None] * J[l][None, :]
    return off, GJ, J
