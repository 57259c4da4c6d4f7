"""Inputs, scalings and restatement runs of the range-edge tests of the batched families, mi355x_qr.h sections 8c to 8n (helper module, no
fixtures, no GPU): tests/test_batched_range_edges_ref.py runs the float64 restatements on them, tests/test_gpu_batched_range_edges.py the
kernels.

A scale pair (ea, eb) multiplies every matrix-like input (A, J, R, C and G with A, the rows pushed into an accumulator, the triangle and
the block of an update) by 2^ea and every right-hand-side-like input (b, f, z, d of gglse, h of lsei; rss by 2^(2 eb)) by 2^eb.  What
follows from them -- a radius, bounds on x, a start, a lambda, a fixed IRLS scale -- is scaled by the exact power of two that keeps the
problem the same problem; caller-supplied scaling vectors D and d stay of order 1.  A pair is admissible for an entry point when every
input, every returned output and every product of one A-like and one b-like quantity has its true value inside 2^+-1000.

Every family runs on a batch of BATCH = 5 members, read-only, computed once.  One member is graded: member 2 has its singular values
graded to a condition of 1e6 in 8d, 8e, 8f, 8g, the triangles of 8k, and the linear batches of 8m and 8n (batched_trust_ref.batch,
batched_minnorm_ref.cond_matrix or the same construction); 8c has members 1 and 3 of its family's cond1e6 class; 8h takes
batched_lse_ref.case, which grades A of members 1 and 4 and C of member 2 to 1e6; 8i, 8j, 8k's fits and 8l take their families' own
batches, which grade members 1 and 4 to 1e4, as those families' tests do.  One member has an exactly zero column where the family
takes one.  Beside the inputs a family has what scales them (`<family>_scaled(inputs, ea, eb)`, or the products written out in
`<family>_ref`) and the exponents by which each floating output is de-scaled (`descale`).  `<family>_ref` is the float64 restatement
on the scaled inputs, its floating outputs already de-scaled (an exact operation).
"""
import functools

import numpy as np

import batched_bvls_ref as BV
import batched_damped_ref as DR
import batched_irls_ref as IR
import batched_lm_ref as L
import batched_lmb_ref as LB
import batched_lse_ref as LSE
import batched_lsei_ref as LSEI
import batched_minnorm_ref as MN
import batched_stats_ref as ST
import batched_svd_ref as SV
import batched_trust_ref as T
import batched_update_ref as UP
import hp_ref as H

EPS = H.EPS
BATCH = 5
E = 480
PAIRS = ((E, 0), (-E, 0), (0, E), (0, -E), (E, E), (-E, -E), (300, 300), (-300, -300))
JOINT = tuple(p for p in PAIRS if p[0] == p[1])
RTOL = 1e-9                   # the restatement scaled and de-scaled against the restatement unscaled


def p2(e):
    return float(np.ldexp(1.0, int(e)))


def tag(pair):
    return f"(2^{pair[0]}, 2^{pair[1]})"


def descale(v, e):
    """v / 2^e, exactly; v must be finite"""
    v = np.asarray(v, dtype=np.float64)
    assert np.isfinite(v).all(), "a non-finite output"
    return np.ldexp(v, -int(e))


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def compare(base, got, what):
    """integer outputs equal, floating outputs (de-scaled) within RTOL of the unscaled run's, member by member (max norm)"""
    bi, bf = base
    gi, gf = got
    assert sorted(bi) == sorted(gi) and sorted(bf) == sorted(gf)
    for k in bi:
        assert np.array_equal(np.asarray(bi[k]), np.asarray(gi[k])), (what, k, bi[k], gi[k])
    for k in bf:
        x, y = np.asarray(bf[k], dtype=np.float64), np.asarray(gf[k], dtype=np.float64)
        assert x.shape == y.shape and np.isfinite(y).all(), (what, k)
        for q in range(x.shape[0]):
            err, ref = np.max(np.abs(x[q] - y[q]), initial=0.0), np.max(np.abs(x[q]), initial=0.0)
            assert err <= RTOL * ref, (what, k, q, err, ref)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8g: the trust-region search from factors.  X ~ 2^(eb - ea), lambda ~ 2^ea, |D x| ~ 2^(eb - ea), resid ~ 2^eb; Delta ~ 2^(eb - ea)
# ----------------------------------------------------------------------------------------------------------------------------------
TRUST_ORDERS = (15, 33)       # the smallest order >= 7 of batched_trust_ref.ORDERS on the wave route; the first of the workgroup route
TRUST_RTOL = 1e-3
TRUST_ZERO = 3                # the member with an exactly zero column (its fraction of the Gauss-Newton |D x|: 1e-2)


@functools.lru_cache(maxsize=None)
def trust_inputs(n):
    """batched_trust_ref.batch(n + 3, n, 5) and its float64 factors; member 2 graded; column n - 3 of member TRUST_ZERO's triangle is
    zero, so R(n-3, n-3) == 0 there: the Gauss-Newton step solves the leading block and the search starts from parl = 0"""
    A, b, d = T.batch(n + 3, n, BATCH)
    fac = [T.factors(A[q], b[q]) for q in range(BATCH)]
    R, z, rss = np.stack([f[0] for f in fac]), np.stack([f[1] for f in fac]), np.array([f[2] for f in fac])
    c = n - 3
    R[TRUST_ZERO][:, c] = 0.0
    A = A.copy()
    A[TRUST_ZERO][:, c] = 0.0
    frac = np.array([T.FRACS[q % len(T.FRACS)] for q in range(BATCH)])
    gn = np.array([T.gauss_newton_dxnorm(R[q][:c, :c], z[q][:c], d[q][:c]) if q == TRUST_ZERO else T.gauss_newton_dxnorm(R[q], z[q], d[q])
                   for q in range(BATCH)])
    delta = frac * gn
    frozen(A, b, d, R, z, rss, delta)
    return dict(A=A, b=b, d=d, R=R, z=z, rss=rss, delta=delta, n=n)


def trust_scaled(p, ea, eb):
    sa, sb = p2(ea), p2(eb)
    return dict(p, A=sa * p["A"], b=sb * p["b"], R=sa * p["R"], z=sb * p["z"], rss=sb * sb * p["rss"], delta=p["delta"] * sb / sa)


def trust_descaled(out, ea, eb):
    """(ints, floats) of a call's dict(X, lam, xnorm, resid, iter, status, info)"""
    ints = {k: np.asarray(out[k]) for k in ("iter", "status", "info")}
    floats = dict(X=descale(out["X"], eb - ea), lam=descale(out["lam"], ea), xnorm=descale(out["xnorm"], eb - ea), resid=descale(out["resid"], eb))
    return ints, floats


def trust_ref(p, ea, eb, search=T.lmpar):
    s = trust_scaled(p, ea, eb)
    res = [search(s["R"][q], s["z"][q], s["delta"][q], s["d"][q], rss=s["rss"][q], rtol=TRUST_RTOL) for q in range(BATCH)]
    assert all(r["info"] == 0 for r in res), [r["info"] for r in res]
    return trust_descaled({k: np.stack([np.asarray(r[k], dtype=np.float64 if k in ("X", "lam", "xnorm", "resid") else np.int64) for r in res])
                           for k in T_KEYS}, ea, eb)


T_KEYS = ("X", "lam", "xnorm", "resid", "iter", "status", "info")


def named_rank_deficient():
    """the member of the defect's report: batched_trust_ref.batch(20, 7, 3, 0, False), member 0, column 4 of the triangle zeroed;
    Delta = 0.5, rtol = 1e-3: (R, z)"""
    A, b, _ = T.batch(20, 7, 3, 0, False)
    R, z, _ = T.factors(A[0], b[0])
    R = R.copy()
    R[:, 4] = 0.0
    return R, z


# ----------------------------------------------------------------------------------------------------------------------------------
# 8m and 8n: f and J scaled jointly by 2^e.  Mode 1 (D from the columns of J): D, Delta, |D x|, |D p| and |f| ~ 2^e, par and the
# cosines scale-free.  Mode 2 (the caller's D, of order 1): |f| ~ 2^e, par ~ 2^(2 e), the rest scale-free.
# ----------------------------------------------------------------------------------------------------------------------------------
LM_SHAPES = ((64, 31), (64, 32))          # batched_lm_ref.LINEAR_SHAPES: the last wave shape (n >= 7), the first workgroup shape
LM_ZERO = 3
LM_FLOATS = ("x", "xtrial", "D") + L.SCALARS
# factor: the first radius is a tenth of |D x0|, so the first searches iterate (with the default 100 the Gauss-Newton step is accepted
# at once and the search never forms the gradient norm)
LM_OPTIONS = dict(gtol=1e-8, factor=0.1)


class Scaled:
    """a problem with f and J multiplied by 2^e"""

    def __init__(self, problem, e):
        self.p, self.s = problem, p2(e)
        self.m, self.n, self.name = problem.m, problem.n, problem.name

    def f(self, xp, x, data):
        return self.s * self.p.f(xp, x, data)

    def jac(self, xp, x, data):
        return self.s * self.p.jac(xp, x, data)


@functools.lru_cache(maxsize=None)
def lm_linear(m, n):
    """(problem, x0, data, lo, hi, unit): five members of batched_lmb_ref.LinearBox(m, n) without a fixed parameter, f = A x - b; member 2 has
    the singular values of A graded to condition 1e6, member LM_ZERO has column n - 3 of A exactly zero and starts with x0 = 0 there (so
    that the scaling MINPACK gives a zero column in mode 1, D_j = 1, multiplies a zero).  lo, hi: the problem's box, which cuts off about
    half of the free minimiser's entries.  unit: the entries of D that mode 1 leaves at 1 whatever the scale (the zero column's)"""
    prob = LB.LinearBox(m, n, BATCH, fix=False)
    x0, data, lo, hi = prob.members(BATCH)
    x0, data = x0.copy(), data.copy()
    A = data[:, :m * n].reshape(BATCH, n, m).transpose(0, 2, 1).copy()
    u, _, vt = np.linalg.svd(A[2], full_matrices=False)
    A[2] = (u * (np.linalg.norm(A[2], 2) * np.logspace(0, -6, n))) @ vt
    A[LM_ZERO][:, n - 3] = 0.0
    x0[LM_ZERO, n - 3] = 0.0
    lo, hi = lo.copy(), hi.copy()
    lo[LM_ZERO, n - 3] = -1.0                      # (x0 = 0 lies inside)
    data[:, :m * n] = A.transpose(0, 2, 1).reshape(BATCH, m * n)
    unit = np.zeros((BATCH, n), dtype=bool)
    unit[LM_ZERO, n - 3] = True
    frozen(x0, data, lo, hi, unit)
    return prob, x0, data, lo, hi, unit


@functools.lru_cache(maxsize=None)
def lm_nonlinear(bounded):
    """(problem, x0, data, lo, hi, None) of expdecay16 (8m) or expdecay_b (8n: the rate's upper bound becomes active), five members.
    expdecay16's data is its planted curve plus noise of 1e-2: with the exact curve |f| goes to rounding at the solution, and the square
    of a rounding-sized f times 2^-480 is below the double range, which no scale pair's admissibility covers"""
    if bounded:
        prob = LB.PROBLEMS["expdecay_b"]
        x0, data, lo, hi, _, _ = LB.good_members(prob, BATCH)
        return prob, x0, data, lo, hi, None
    prob = L.PROBLEMS["expdecay16"]
    x0, data, _ = prob.members(BATCH)
    data = data + 0.02 * DR.U(160016, BATCH, prob.m)
    frozen(data)
    return prob, x0, data, None, None, None


def lm_exponents(mode, e):
    """the exponent of every floating state array under f, J -> 2^e f, 2^e J"""
    ex = dict.fromkeys(LM_FLOATS + ("alpha",), 0)
    ex["fnorm"] = e
    if mode == 2:
        ex["par"] = 2 * e
    else:
        for k in ("D", "delta", "xnorm", "pnorm"):
            ex[k] = e
    return ex


def lm_descaled(state, mode, e, bounded, unit=None):
    """(ints, floats) of a final state: dict of arrays with a leading batch axis"""
    ex = lm_exponents(mode, e)
    ints = {k: np.asarray(state[k]) for k in L.COUNTERS + (("peg", "clipped") if bounded else ())}
    floats = {k: descale(state[k], ex[k]) for k in LM_FLOATS + (("alpha",) if bounded else ())}
    if unit is not None and mode != 2:
        floats["D"] = np.where(unit, np.asarray(state["D"], dtype=np.float64), floats["D"])
    return ints, floats


def lm_options(prob, mode, linear):
    o = dict(prob.options)
    if linear:
        o.update(LM_OPTIONS)
    o["mode"] = mode
    return o


def lm_ref(case, e, mode, bounded):
    prob, x0, data, lo, hi, unit = case
    sp = Scaled(prob, e)
    o = lm_options(prob, mode, isinstance(prob, LB.LinearBox))
    mem = []
    for q in range(BATCH):
        D0 = np.ones(prob.n) if mode == 2 else None
        dq = None if data is None else data[q]
        if bounded:
            mem.append(LB.solve(sp, x0[q], dq, lo[q], hi[q], np.float64, D0, **o))
        else:
            mem.append(L.solve(sp, x0[q], dq, np.float64, D0, **o)[0])
    keys = LM_FLOATS + L.COUNTERS + (("peg", "clipped", "alpha") if bounded else ())
    state = {k: np.stack([np.asarray(getattr(m, k)) for m in mem]) for k in keys}
    return lm_descaled(state, mode, e, bounded, unit)


def stack(res, keys, dtype):
    return {k: np.stack([np.asarray(r[k], dtype=dtype) for r in res]) for k in keys}


# ----------------------------------------------------------------------------------------------------------------------------------
# 8i: x, lo, hi ~ 2^(eb - ea), w = A^T (b - A x) ~ 2^(ea + eb), resid ~ 2^eb
# ----------------------------------------------------------------------------------------------------------------------------------
BVLS_SHAPES = ((8, 7), (65, 31))          # batched_bvls_ref: the smallest wave shape with n >= 7, the first workgroup shape


def bvls_scaled(c, ea, eb):
    sa, sb = p2(ea), p2(eb)
    return dict(A=sa * c["A"], b=sb * c["b"], lo=c["lo"] * sb / sa, hi=c["hi"] * sb / sa)


def bvls_descaled(out, ea, eb):
    return ({k: np.asarray(out[k]) for k in ("state", "iter", "info")},
            dict(x=descale(out["x"], eb - ea), w=descale(out["w"], ea + eb), resid=descale(out["resid"], eb)))


def bvls_ref(shape, ea, eb):
    s = bvls_scaled(BV.case(*shape, batch=BATCH), ea, eb)
    res = [BV.bvls(s["A"][q], s["b"][q], s["lo"][q], s["hi"][q]) for q in range(BATCH)]
    return bvls_descaled(dict(stack(res, ("x", "w", "resid"), np.float64), **stack(res, ("state", "iter", "info"), np.int64)), ea, eb)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8l: G with A, h with b: x ~ 2^(eb - ea); mu, s and resid ~ 2^eb
# ----------------------------------------------------------------------------------------------------------------------------------
LSEI_SHAPES = ((8, 7, 3, 1), (65, 31, 10, 0))         # with an equality on the wave route, without on the workgroup route


def lsei_scaled(c, ea, eb):
    sa, sb = p2(ea), p2(eb)
    return dict(A=sa * c["A"], b=sb * c["b"], G=sa * c["G"], h=sb * c["h"])


def lsei_descaled(out, ea, eb):
    return ({k: np.asarray(out[k]) for k in ("state", "iter", "info")},
            dict(x=descale(out["x"], eb - ea), mu=descale(out["mu"], eb), s=descale(out["s"], eb), resid=descale(out["resid"], eb)))


def lsei_ref(shape, ea, eb):
    s = lsei_scaled(LSEI.case(*shape, batch=BATCH), ea, eb)
    res = [LSEI.lsei(s["A"][q], s["b"][q], s["G"][q], s["h"][q], shape[3]) for q in range(BATCH)]
    return lsei_descaled(dict(stack(res, ("x", "mu", "s", "resid"), np.float64), **stack(res, ("state", "iter", "info"), np.int64)), ea, eb)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8h: C with A, d with b: x ~ 2^(eb - ea); lambda and resid ~ 2^eb
# ----------------------------------------------------------------------------------------------------------------------------------
LSE_SHAPES = ((16, 8, 3, 1), (65, 31, 7, 1))


def lse_scaled(c, ea, eb):
    sa, sb = p2(ea), p2(eb)
    return dict(A=sa * c["A"], C=sa * c["C"], B=sb * c["B"], D=sb * c["D"])


def lse_descaled(out, ea, eb):
    return ({"info": np.asarray(out["info"])},
            dict(X=descale(out["X"], eb - ea), lam=descale(out["lam"], eb), resid=descale(out["resid"], eb)))


def lse_ref(shape, ea, eb):
    s = lse_scaled(LSE.case(*shape, batch=BATCH), ea, eb)
    res = [LSE.gglse(s["A"][q], s["C"][q], s["B"][q], s["D"][q], np.float64) for q in range(BATCH)]
    out = dict(X=np.stack([r[0] for r in res]), lam=np.stack([r[1] for r in res]), resid=np.stack([r[2] for r in res]), info=np.zeros(BATCH, dtype=np.int64))
    return lse_descaled(out, ea, eb)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8j: x ~ 2^(eb - ea); the scale s and resid ~ 2^eb; the weights scale-free.  A fixed scale is a b-like input.
# ----------------------------------------------------------------------------------------------------------------------------------
IRLS_SHAPES = ((16, 7), (65, 15))
IRLS_LOSSES = (IR.HUBER, IR.BISQUARE)


def irls_scaled(c, ea, eb):
    return dict(A=p2(ea) * c["A"], b=p2(eb) * c["b"])


def irls_descaled(out, ea, eb):
    return ({k: np.asarray(out[k]) for k in ("iter", "status", "info")},
            dict(x=descale(out["x"], eb - ea), w=descale(out["w"], 0), s=descale(out["s"], eb), resid=descale(out["resid"], eb)))


def irls_ref(shape, loss, ea, eb):
    s = irls_scaled(IR.case(*shape, loss, batch=BATCH), ea, eb)
    res = [IR.irls(s["A"][q], s["b"][q], loss, tol=IR.TOL) for q in range(BATCH)]
    return irls_descaled(dict(stack(res, ("x", "w", "s", "resid"), np.float64), **stack(res, ("iter", "status", "info"), np.int64)), ea, eb)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8k: x and se ~ 2^(eb - ea), e ~ 2^eb, sigma2 ~ 2^(2 eb), the leverages scale-free, C ~ 2^(2 eb - 2 ea) (unscaled: 2^(-2 ea))
# ----------------------------------------------------------------------------------------------------------------------------------
STATS_SHAPES = ((16, 8), (64, 32))
STATS_TRI = (8, 33)           # covariance from a triangle: one order per route; member 3 has rank n - 1 (a zero last column after pivoting)


def stats_scaled(shape, ea, eb):
    A, b, p = ST.make_case(*shape, True, BATCH)
    return p2(ea) * A, p2(eb) * b, p


def stats_descaled(out, ea, eb):
    return ({k: np.asarray(out[k]) for k in ("dof", "info")},
            dict(x=descale(out["x"], eb - ea), e=descale(out["e"], eb), h=descale(out["h"], 0), sigma2=descale(out["sigma2"], 2 * eb),
                 C=descale(out["C"], 2 * eb - 2 * ea), se=descale(out["se"], eb - ea)))


def stats_ref(shape, ea, eb):
    A, b, p = stats_scaled(shape, ea, eb)
    res = [ST.fit_stats(A[q], b[q], p[q], True) for q in range(BATCH)]
    return stats_descaled(dict(stack(res, ("x", "e", "h", "sigma2", "C", "se"), np.float64), **stack(res, ("dof", "info"), np.int64)), ea, eb)


@functools.lru_cache(maxsize=None)
def tri_inputs(n):
    """pivoted float64 factors of five (n + 5) x n members of batched_trust_ref.batch (member 2 graded); member 3 has column 1 exactly
    zero: it is pivoted last, R(n-1, n-1) == 0 and its rank is n - 1.  (R, jpvt, rank)"""
    A, _, _ = T.batch(n + 5, n, BATCH, 3)
    A = A.copy()
    A[3][:, 1] = 0.0
    R, jp, rank = [], [], []
    for q in range(BATCH):
        F, _, j = H.qrp(A[q], np.float64)
        Rq = np.triu(np.asarray(F[:n], dtype=np.float64))
        if q == 3:
            assert j[n - 1] == 1 and np.all(Rq[:, n - 1] == 0.0)
        R.append(Rq), jp.append(np.asarray(j)), rank.append(n - 1 if q == 3 else n)
    R, jp, rank = np.stack(R), np.stack(jp), np.array(rank)
    frozen(R, jp, rank)
    return R, jp, rank


def tri_ref(n, ea):
    R, jp, rank = tri_inputs(n)
    res = [ST.covar_from_r(p2(ea) * R[q], jp[q], rank[q]) for q in range(BATCH)]
    return {}, dict(C=descale(np.stack([r[0] for r in res]), -2 * ea), se=descale(np.stack([r[1] for r in res]), -ea))


# ----------------------------------------------------------------------------------------------------------------------------------
# 8f: lambda is A-like (it damps in the units of A), d stays: X and |D x| ~ 2^(eb - ea), resid ~ 2^eb
# ----------------------------------------------------------------------------------------------------------------------------------
DAMPED_SHAPES = ((17, 17, 1), (64, 32, 1))
DAMPED_WIDE = ((7, 6), (100, 33))         # as the tall F (rows, cols) the wide member is the transpose of
DAMPED_TRI = (15, 33)


def damped_descaled(out, ea, eb):
    return ({"info": np.asarray(out["info"])},
            dict(X=descale(out["X"], eb - ea), xnorm=descale(out["xnorm"], eb - ea), resid=descale(out["resid"], eb)))


def _damped_pack(res):
    """a list over members of lists over lambdas of (X, xnorm, resid, info) -> dict of (b, nlam, ...) arrays"""
    assert all(r[3] == 0 for m in res for r in m)
    return dict(X=np.stack([np.stack([r[0] for r in m]) for m in res]), xnorm=np.stack([np.stack([r[1] for r in m]) for m in res]),
                resid=np.stack([np.stack([r[2] for r in m]) for m in res]), info=np.zeros((len(res), len(res[0])), dtype=np.int64))


GRADED = 2                    # the member that is graded


@functools.lru_cache(maxsize=None)
def damped_inputs(m, n, nrhs, with_d):
    """batched_damped_ref.case(m, n, nrhs, with_d, 5) with member GRADED's A replaced by a matrix whose singular values are graded from 1
    to 1e-6 (batched_minnorm_ref.cond_matrix, the construction the families' conditioned cases use), its lambdas, truth, float64
    measures and caps recomputed as batched_damped_ref.case computes them"""
    c = DR.case(m, n, nrhs, with_d, BATCH)
    q = GRADED
    A, lam = c["A"].copy(), c["lam"].copy()
    A[q] = MN.cond_matrix(max(m, n), min(m, n), 1e6, 4242 + 100 * m + n) if m >= n else MN.cond_matrix(n, m, 1e6, 4242 + 100 * m + n).T
    lam[q] = DR.lam_list(A[q], m, n)
    dq = None if c["d"] is None else c["d"][q]
    r64 = DR.tall(A[q], c["B"][q], lam[q], dq) if m >= n else DR.wide(A[q], c["B"][q], lam[q])
    assert all(r[3] == 0 for r in r64)
    Tq = [DR.truth(A[q], c["B"][q], l, dq) for l in lam[q]]
    rq = [DR.measures(A[q], c["B"][q], l, dq, r64[k][0], r64[k][1], r64[k][2], Tq[k]) for k, l in enumerate(lam[q])]
    cq = [DR.caps(A[q], c["B"][q], l, dq, Tq[k]) for k, l in enumerate(lam[q])]
    frozen(A, lam)
    swap = lambda full, mine: [mine if i == q else full[i] for i in range(BATCH)]
    return dict(c, A=A, lam=lam, T=swap(c["T"], Tq), ref=swap(c["ref"], rq), caps=swap(c["caps"], cq))


def damped_ref(shape, ea, eb):
    c = damped_inputs(*shape, True)
    sa, sb = p2(ea), p2(eb)
    return damped_descaled(_damped_pack([DR.tall(sa * c["A"][q], sb * c["B"][q], sa * c["lam"][q], c["d"][q]) for q in range(BATCH)]), ea, eb)


def damped_wide_ref(shape, ea, eb):
    rows, cols = shape
    c = damped_inputs(cols, rows, 1, False)
    sa, sb = p2(ea), p2(eb)
    return damped_descaled(_damped_pack([DR.wide(sa * c["A"][q], sb * c["B"][q], sa * c["lam"][q][:3]) for q in range(BATCH)]), ea, eb)


@functools.lru_cache(maxsize=None)
def damped_tri_inputs(n):
    """pivoted float64 factors of the members of batched_trust_ref.batch(n + 3, n, 5): dict(A, B, d, lam (b, 3), R, Z, rss, jpvt); member
    2 graded, column 1 of member 3 exactly zero (pivoted last: R(n-1, n-1) == 0, which every lambda > 0 damps)"""
    m = n + 3
    A, b, d = T.batch(m, n, BATCH, 5)
    A = A.copy()
    A[3][:, 1] = 0.0
    R, Z, rss, jp = [], [], [], []
    for q in range(BATCH):
        F, tau, j = H.qrp(A[q], np.float64)
        y = np.asarray(H.apply_q(F, tau, b[q][:, None], "T", np.float64), dtype=np.float64)
        R.append(np.triu(np.asarray(F[:n], dtype=np.float64))), Z.append(y[:n]), rss.append((y[n:] ** 2).sum(axis=0)), jp.append(np.asarray(j))
    lam = np.stack([np.array([1e-8, 0.3, 30.0]) * np.linalg.norm(A[q], 2) for q in range(BATCH)])
    out = dict(A=A, B=b[:, :, None].copy(), d=d, lam=lam, R=np.stack(R), Z=np.stack(Z), rss=np.stack(rss), jpvt=np.stack(jp))
    frozen(*out.values())
    assert np.all(out["R"][3][:, n - 1] == 0.0)
    return out


def damped_tri_ref(n, ea, eb):
    c = damped_tri_inputs(n)
    sa, sb = p2(ea), p2(eb)
    res = [[DR.solve(sa * c["R"][q], sb * c["Z"][q], sa * l, c["d"][q], c["jpvt"][q], sb * sb * c["rss"][q]) for l in c["lam"][q]] for q in range(BATCH)]
    return damped_descaled(_damped_pack(res), ea, eb)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8e: the wide system F^T X = B: X ~ 2^(eb - ea)
# ----------------------------------------------------------------------------------------------------------------------------------
MINNORM_SHAPES = ((17, 17, 1), (64, 32, 40))


@functools.lru_cache(maxsize=None)
def minnorm_inputs(shape):
    """batched_minnorm_ref.case(*shape, "U", 5) with member GRADED replaced by the first member of the family's graded kind, "cond"
    (cond_matrix at 1e6), that the family's quarter rule keeps, with its own truth, float64 measures and caps; kind: the kind per member"""
    c = MN.case(*shape, "U", BATCH)
    seed = 1000 * shape[0] + 10 * shape[1] + shape[2] + 31
    g = next(m for m in (MN.member(*shape, "cond", seed + 7919 * t) for t in range(250)) if MN.quarter(m))
    swap = lambda k: [g[k] if q == GRADED else c[k][q] for q in range(BATCH)]
    F, B = np.stack(swap("F")), np.stack(swap("B"))
    frozen(F, B)
    return dict(F=F, B=B, Xld=swap("Xld"), ref=swap("ref"), caps=swap("caps"), kind=["cond" if q == GRADED else "U" for q in range(BATCH)])


def minnorm_ref(shape, ea, eb):
    c = minnorm_inputs(shape)
    X = np.stack([np.asarray(H.minnorm(np.ascontiguousarray(p2(ea) * c["F"][q].T), p2(eb) * c["B"][q], np.float64), dtype=np.float64) for q in range(BATCH)])
    return {}, dict(X=descale(X, eb - ea))


# ----------------------------------------------------------------------------------------------------------------------------------
# 8c: S ~ 2^ea, U and V scale-free
# ----------------------------------------------------------------------------------------------------------------------------------
SVD_SHAPES = ((8, 8), (65, 33))
# (there is no right-hand side: the pairs with ea == 0 are the unscaled run, and a joint pair is the run of its first exponent)
SVD_PAIRS = tuple((e, 0) for e in sorted({p[0] for p in PAIRS if p[0]}, key=lambda e: (-abs(e), -e)))


@functools.lru_cache(maxsize=None)
def svd_inputs(m, n):
    """five members of batched_svd_ref: gaussian, cond1e6, zerodup (column 1 exactly zero, the last a copy of the first), cond1e6,
    gaussian"""
    g, c, z = (SV.make_batch(k, m, n, BATCH)[0] for k in ("gaussian", "cond1e6", "zerodup"))
    A = np.stack([g[0], c[1], z[2], c[3], g[4]])
    frozen(A)
    return A


def svd_ref(shape, ea):
    A0 = svd_inputs(*shape)
    A = p2(ea) * A0
    S, rank, sweeps = [], [], []
    for q in range(BATCH):
        F, tau, jp = SV.dlaqp2(A[q])
        s, v, w, r, sw = SV.jsvd_ref(F, jp)
        # the section's four bounds on the de-scaled factors: reconstruction, sigma, |V^T V - I| and |U^T U - I| with U = Q W
        SV.check_bounds(A0[q], SV.form_q(F, tau) @ w, descale(s, ea), v, sw)
        S.append(s), rank.append(r), sweeps.append(sw)
    # (V only up to the sign of a column and, for the zero singular values, up to a rotation: across scales the values and the counts are compared)
    return dict(rank=np.array(rank), sweeps=np.array(sweeps)), dict(S=descale(np.stack(S), ea))


# ----------------------------------------------------------------------------------------------------------------------------------
# 8d: the triangle and the block ~ 2^ea, the right-hand sides ~ 2^eb: R' ~ 2^ea, V and tau scale-free, C' ~ 2^eb; the accumulator's
# X ~ 2^(eb - ea), rss ~ 2^(2 eb)
# ----------------------------------------------------------------------------------------------------------------------------------
UPDATE_SHAPES = ((15, 6), (33, 6))        # (n, p): half of the block's rows added, half removed


@functools.lru_cache(maxsize=None)
def update_inputs(n, p):
    """five members: X0 (2 n + p rows, member 2 graded) whose last p / 2 rows are removed while p / 2 new rows are added; right-hand
    sides of two columns.  dict(X0, Y0, R, Z, B, C2, p_add)"""
    rows, half = 2 * n + p, p // 2
    X0, _, _ = T.batch(rows, n, BATCH, 7)
    Y0 = DR.U(7000 + n, BATCH, rows, 2)
    new, newy = DR.U(7100 + n, BATCH, half, n), DR.U(7200 + n, BATCH, half, 2)
    R, Z = [], []
    for q in range(BATCH):
        Q, Rq = np.linalg.qr(X0[q])
        R.append(np.triu(Rq)), Z.append(Q.T @ Y0[q])
    B = np.concatenate([new, X0[:, rows - half:]], axis=1)
    C2 = np.concatenate([newy, Y0[:, rows - half:]], axis=1)
    out = dict(X0=X0, Y0=Y0, R=np.stack(R), Z=np.stack(Z), B=B, C2=C2)
    frozen(*out.values())
    return dict(out, p_add=half, n=n, p=p)


def update_descaled(out, ea, eb):
    return ({"info": np.asarray(out["info"])},
            dict(R=descale(out["R"], ea), V=descale(out["V"], 0), tau=descale(out["tau"], 0), C1=descale(out["C1"], eb), C2=descale(out["C2"], eb)))


def update_ref(shape, ea, eb):
    c = update_inputs(*shape)
    sa, sb = p2(ea), p2(eb)
    res = [UP.update(sa * c["R"][q], sa * c["B"][q], c["p_add"], sb * c["Z"][q], sb * c["C2"][q]) for q in range(BATCH)]
    out = dict(R=np.stack([np.triu(r[0]) for r in res]), V=np.stack([r[1] for r in res]), tau=np.stack([r[2] for r in res]),
               C1=np.stack([r[3] for r in res]), C2=np.stack([r[4] for r in res]), info=np.array([r[5] for r in res]))
    return update_descaled(out, ea, eb)


def acc_plan(c):
    """the accumulator's life on update_inputs: push the first 2 n rows, push p more, pop the p / 2 oldest, slide (p / 2 new in, the
    next p / 2 oldest out): (call, new rows or None, old rows or None) as index ranges into X0 / (B, C2)"""
    n, p, half = c["n"], c["p"], c["p_add"]
    return (("push", (0, 2 * n), None), ("push", (2 * n, 2 * n + p), None), ("pop", None, (0, half)), ("slide", "new", (half, 2 * half)))


def acc_ref(shape, ea, eb):
    c = update_inputs(*shape)
    sa, sb = p2(ea), p2(eb)
    n, half = c["n"], c["p_add"]
    X, rss, rows, infos = [], [], [], []
    for q in range(BATCH):
        A, Y = sa * c["X0"][q], sb * c["Y0"][q]
        new, newy = sa * c["B"][q][:half], sb * c["C2"][q][:half]
        acc = UP.Accumulator(n, 2)
        info = []
        for call, a, o in acc_plan(c):
            An, Yn = (new, newy) if a == "new" else ((A[a[0]:a[1]], Y[a[0]:a[1]]) if a else (A[:0], Y[:0]))
            Ao, Yo = (A[o[0]:o[1]], Y[o[0]:o[1]]) if o else (A[:0], Y[:0])
            info.append(acc.step(An, Yn, Ao, Yo))
        X.append(H.solve_r(np.triu(acc.R), acc.Z, np.float64)), rss.append(acc.rss), rows.append(acc.rows), infos.append(info)
    return dict(rows=np.array(rows), info=np.array(infos)), dict(X=descale(np.stack(X), eb - ea), rss=descale(np.stack(rss), 2 * eb))
