"""-m gpu: the batched trust-region step (mi355x_qr.h section 8g), member by member.

Inputs, radii and the restatement: tests/batched_trust_ref.py.  Delta = f x the Gauss-Newton |D x| with f cycling over (2, 1.05, 0.5,
1e-2, 1e-6) by member, so the waves of one workgroup run 0 to several iterations side by side; every third member is graded to condition
1e6.  The orders cover every wave width, both edges of the wave route (n + 1 = 32 and 33) and the LDS limit of the workgroup route (63).

What ties the search to a kernel already verified: X, xnorm and resid of a member are bitwise qr_damped_batched_dev's for the lambda the
search returns.  What ties it to the problem: the returned |D x| meets the termination rule exactly (the kernel decided on that number),
and |D x| re-evaluated in longdouble from the returned X meets it within the rounding of the norm itself, (n + 4) eps |D x| -- the
`rows eps` term of the damped call's xnorm cap, the only part of that cap that applies to a norm taken of the same X.

Iteration counts are printed (-s) and tabulated in DESIGN.md section 7n; they are asserted only to stay within maxit, and status 3
(maxit reached) never to occur."""
import numpy as np
import pytest
import torch

import batched_trust_ref as T
import hp_ref as H
from test_gpu_batched_damped import SENTINEL, Shared, Strided, _damped, _fused, _gels, _wide

pytestmark = pytest.mark.gpu

KEYS = ("X", "lam", "xnorm", "resid", "iter", "status", "info")


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


def _dev(v, dtype=torch.float64):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dtype).cuda()


class Out:
    """the outputs of one call, sentinel-filled"""

    def __init__(self, xrows, b):
        self.X = Strided(xrows, 1, b)
        self.lam, self.xn, self.rs = (torch.full((b,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(3))
        self.it, self.st, self.info = (torch.full((b,), 77, dtype=torch.int32, device="cuda") for _ in range(3))
        torch.cuda.synchronize()

    def kw(self):
        return dict(dxnorm=self.xn, dresid=self.rs, diter=self.it, dstatus=self.st)

    def collect(self):
        return dict(X=self.X.get()[:, :, 0], lam=self.lam.cpu().numpy(), xnorm=self.xn.cpu().numpy(), resid=self.rs.cpu().numpy(),
                    iter=self.it.cpu().numpy(), status=self.st.cpu().numpy(), info=self.info.cpu().numpy())


def _per_member(v, shared):
    """(pointer, stride) of one double per member; shared: member 0's for everybody at stride 0"""
    if v is None:
        return None, 0, None
    t = _dev(v[:1] if shared else v)
    return t, 0 if shared else 1, t


def _vecs(d, shared):
    if d is None:
        return None, 0, None
    x = Shared(d[0]) if shared else Strided(d.shape[1], 1, d.shape[0], d[:, :, None])
    return x.ptr, x.stride, x


def _trust(plan, R, z, delta, d=None, rss=None, jpvt=None, flip=False, lam0=None, rtol=0.1, maxit=T.MAXIT, shared=False):
    """qr_trust_batched_dev on R (batch, n, n; what lies below the diagonal is not read) and z (batch, n)"""
    b, n, _ = R.shape
    dR, dZ, o = Strided(n, n, b, R), Strided(n, 1, b, z[:, :, None]), Out(n, b)
    Dp, Ds, _k1 = _vecs(d, shared)
    dj = None if jpvt is None else Strided(n, 1, b, jpvt[:, :, None].astype(np.int32), dtype=np.int32)
    delp, dels, _k2 = _per_member(delta, shared)
    l0p, l0s, _k3 = _per_member(lam0, False)
    plan.trust_batched(dR.ptr, n, dR.ld, dR.stride, dZ.ptr, dZ.ld, dZ.stride, delp, dels, o.X.ptr, o.X.ld, o.X.stride, o.lam, o.info, b,
                       drss=_dev(rss), djpvt=None if dj is None else dj.ptr, stridejpvt=0 if dj is None else dj.stride, dD=Dp, strideD=Ds,
                       dlam0=l0p, stridelam0=l0s, rtol=rtol, maxit=maxit, flip=flip, **o.kw())
    plan.sync()
    assert dR.unchanged() and dZ.unchanged(), "the factors are read only"
    return o.collect()


def _gels_trust(plan, A, bb, delta, d=None, rtol=0.1, maxit=T.MAXIT):
    """qr_gels_trust_batched_dev: the results, and the factors and Q^T b it leaves"""
    b, m, n = A.shape
    dA, dtau, dB, o = Strided(m, n, b, A), Strided(n, 1, b), Strided(m, 1, b, bb[:, :, None]), Out(n, b)
    Dp, Ds, _k = _vecs(d, False)
    delp = _dev(delta)
    plan.gels_trust_batched(dA.ptr, m, n, dA.ld, dA.stride, dtau.ptr, dtau.stride, dB.ptr, dB.ld, dB.stride, delp, 1, o.X.ptr, o.X.ld,
                            o.X.stride, o.lam, o.info, b, dD=Dp, strideD=Ds, rtol=rtol, maxit=maxit, **o.kw())
    plan.sync()
    out = o.collect()
    out.update(F=dA.get(), tau=dtau.get()[:, :, 0], Qtb=dB.get()[:, :, 0])
    return out


def _wide_trust(plan, A, bb, delta, rtol=0.1, maxit=T.MAXIT):
    b, m, n = A.shape
    dA, dF, dtau, dB, o = Strided(m, n, b, A), Strided(n, m, b), Strided(m, 1, b), Strided(m, 1, b, bb[:, :, None]), Out(n, b)
    delp = _dev(delta)
    plan.gels_trust_wide_batched(dA.ptr, m, n, dA.ld, dA.stride, dF.ptr, dF.ld, dF.stride, dtau.ptr, dtau.stride, dB.ptr, dB.ld, dB.stride,
                                 delp, 1, o.X.ptr, o.X.ld, o.X.stride, o.lam, o.info, b, rtol=rtol, maxit=maxit, **o.kw())
    plan.sync()
    assert dA.unchanged() and dB.unchanged(), "the wide matrix, the right-hand side and their padding are untouched"
    return o.collect()


def _same(a, b, keys=KEYS, members=None):
    for k in keys:
        x, y = (a[k], b[k]) if members is None else (a[k][members], b[k][members])
        assert np.array_equal(x, y), k


def _problem(m, n, count, salt=0, with_d=True):
    """members, their float64 factors and the radii: Delta = f x the Gauss-Newton |D x|"""
    A, b, d = T.batch(m, n, count, salt, with_d)
    fac = [T.factors(A[q], b[q]) for q in range(count)]
    R, z, rss = np.stack([f[0] for f in fac]), np.stack([f[1] for f in fac]), np.array([f[2] for f in fac])
    frac = np.array([T.FRACS[q % len(T.FRACS)] for q in range(count)])
    delta = frac * np.array([T.gauss_newton_dxnorm(R[q], z[q], None if d is None else d[q]) for q in range(count)])
    return dict(A=A, b=b, d=d, R=R, z=z, rss=rss, frac=frac, delta=delta)


def _check_rule(tag, out, delta, d, rtol, frac=None, full_rank=True):
    """checks 1, 3 and 4 of a call's outputs"""
    b, n = out["X"].shape[0], (out["X"].shape[1] if d is None else d.shape[1])
    assert np.all(out["info"] == 0), out["info"]
    for q in range(b):
        lam, xn, it, st = out["lam"][q], out["xnorm"][q], out["iter"][q], out["status"][q]
        assert lam >= 0 and T.meets_rule(xn, lam, delta[q], rtol), (tag, q, xn, delta[q], lam)
        dx = H.arr(out["X"][q]) if d is None else H.arr(d[q]) * H.arr(out["X"][q])
        xl = H.norm(dx)
        slack = rtol * delta[q] + T.norm_slack(n) * float(xl)
        assert (xl - delta[q] <= slack) if lam == 0 else (abs(xl - delta[q]) <= slack), (tag, q, float(xl), delta[q])
        assert 0 <= it <= T.MAXIT and (st == 1) == (it == 0) == (lam == 0.0)
        assert st in ((0, 1) if full_rank else (0, 1, 2)), (tag, q, st)
        if frac is not None and frac[q] >= 1.05:
            assert st == 1 and lam == 0.0 and it == 0, (tag, q)
        if frac is not None and frac[q] < 1 and full_rank:
            assert st == 0 and it >= 1 and lam > 0
    print(f"ITER {tag} rtol {rtol}: iterations {out['iter'].tolist()} status {out['status'].tolist()}")


def _check_is_damped(plan, out, R, z, d, rss, jpvt=None, flip=False):
    """check 2: X, xnorm and resid are bitwise qr_damped_batched_dev's with nlam = 1 and the lambda returned"""
    ok = out["info"] == 0
    lam = np.where(ok, out["lam"], 1.0)
    dm = _damped(plan, R, z[:, :, None], d, lam[:, None], None if rss is None else rss[:, None], jpvt=jpvt, flip=flip)
    assert np.array_equal(dm["X"][ok, 0, :, 0], out["X"][ok])
    assert np.array_equal(dm["xnorm"][ok, 0, 0], out["xnorm"][ok]) and np.array_equal(dm["resid"][ok, 0, 0], out["resid"][ok])


# ------------------------------------------------------------------------------------------------
# from factors
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rtol", T.RTOLS)
@pytest.mark.parametrize("n", T.ORDERS)
def test_from_factors(plan, n, rtol):
    count = 9 if n <= 32 else 5
    p = _problem(n + 3, n, count)
    out = _trust(plan, p["R"], p["z"], p["delta"], p["d"], p["rss"], rtol=rtol)
    _check_rule(f"factors n={n}", out, p["delta"], p["d"], rtol, p["frac"])
    _check_is_damped(plan, out, p["R"], p["z"], p["d"], p["rss"])
    # check 7: a repeat, the batch reversed, a member alone
    _same(out, _trust(plan, p["R"], p["z"], p["delta"], p["d"], p["rss"], rtol=rtol))
    rev = _trust(plan, p["R"][::-1], p["z"][::-1], p["delta"][::-1], p["d"][::-1], p["rss"][::-1], rtol=rtol)
    _same(out, {k: v[::-1] for k, v in rev.items()})
    q = 3
    one = _trust(plan, p["R"][q:q + 1], p["z"][q:q + 1], p["delta"][q:q + 1], p["d"][q:q + 1], p["rss"][q:q + 1], rtol=rtol)
    _same({k: v[q:q + 1] for k, v in out.items()}, one)


@pytest.mark.parametrize("n", [15, 33])
def test_shared_operands_and_the_missing_starting_guess(plan, n):
    p = _problem(n + 3, n, 5)
    delta, d = np.repeat(p["delta"][3:4], 5), np.repeat(p["d"][:1], 5, axis=0)        # one small radius, one d for everybody
    rep = _trust(plan, p["R"], p["z"], delta, d, p["rss"], rtol=1e-3)
    assert np.all(rep["info"] == 0) and rep["iter"].max() >= 1
    _same(rep, _trust(plan, p["R"], p["z"], delta, d, p["rss"], rtol=1e-3, shared=True))           # stride 0 for Delta and d
    _same(rep, _trust(plan, p["R"], p["z"], delta, d, p["rss"], rtol=1e-3, lam0=np.zeros(5)))      # dlam0 = NULL is a guess of 0
    nod = _trust(plan, p["R"], p["z"], delta, None, p["rss"], rtol=1e-3)                            # dD = NULL is d = 1
    _same(nod, _trust(plan, p["R"], p["z"], delta, np.ones((5, n)), p["rss"], rtol=1e-3))


@pytest.mark.parametrize("n", [15, 31, 63])
def test_a_bad_radius_fails_its_member_alone(plan, n):
    p = _problem(n + 3, n, 5)
    good = _trust(plan, p["R"], p["z"], p["delta"], p["d"], p["rss"])
    for q, bad in ((0, 0.0), (2, -1.0), (3, float("nan")), (4, float("inf"))):
        delta = p["delta"].copy()
        delta[q] = bad
        out = _trust(plan, p["R"], p["z"], delta, p["d"], p["rss"])
        info = np.zeros(5, dtype=int)
        info[q] = -1
        assert np.array_equal(out["info"], info)
        assert np.all(out["X"][q] == SENTINEL) and out["lam"][q] == SENTINEL and out["xnorm"][q] == SENTINEL and out["resid"][q] == SENTINEL
        assert out["iter"][q] == 77 and out["status"][q] == 77
        _same(out, good, members=[i for i in range(5) if i != q])


# ------------------------------------------------------------------------------------------------
# scaling by a power of two is exact; a warm start
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [15, 33])
def test_scale_equivariance_is_exact(plan, n):
    p = _problem(n + 3, n, 5)
    R, z, d, rss, delta = p["R"], p["z"], p["d"], p["rss"], p["delta"]
    base = _trust(plan, R, z, delta, d, rss, rtol=1e-3)
    assert base["iter"].max() >= 2
    for k in (40, -40):
        s = 2.0 ** k
        o = _trust(plan, s * R, z, delta / s, d, rss, rtol=1e-3)                  # (A, 1 / Delta) scaled
        assert np.array_equal(o["X"], base["X"] / s) and np.array_equal(o["lam"], base["lam"] * s), k
        assert np.array_equal(o["xnorm"], base["xnorm"] / s) and np.array_equal(o["resid"], base["resid"])
        _same(o, base, ("iter", "status", "info"))
        o = _trust(plan, R, s * z, s * delta, d, s * s * rss, rtol=1e-3)          # (b, Delta) scaled
        assert np.array_equal(o["X"], base["X"] * s) and np.array_equal(o["lam"], base["lam"]), k
        assert np.array_equal(o["xnorm"], base["xnorm"] * s) and np.array_equal(o["resid"], base["resid"] * s)
        _same(o, base, ("iter", "status", "info"))


@pytest.mark.parametrize("n", [7, 40])
def test_a_warm_start_takes_no_more_iterations(plan, n):
    p = _problem(n + 3, n, 5)
    cold = _trust(plan, p["R"], p["z"], p["delta"], p["d"], p["rss"], rtol=1e-3)
    warm = _trust(plan, p["R"], p["z"], p["delta"], p["d"], p["rss"], rtol=1e-3, lam0=cold["lam"])
    _check_rule(f"warm n={n}", warm, p["delta"], p["d"], 1e-3, p["frac"])
    assert np.all(warm["iter"] <= cold["iter"]) and np.all((warm["iter"] == 0) == (cold["iter"] == 0))


# ------------------------------------------------------------------------------------------------
# factor and search: the fused launch, the composed route
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rtol", T.RTOLS)
@pytest.mark.parametrize("m,n", [(1, 1), (5, 3), (64, 15), (64, 31), (65, 4), (64, 32), (100, 33), (256, 63)])
def test_factor_and_search(plan, m, n, rtol):
    fused = m <= 64 and n + 1 <= 32
    count = 9 if m * n <= 64 * 32 else 5
    A, b, d = T.batch(m, n, count)
    # the radii need the Gauss-Newton |D x|: from float64 factors on the host (it is only a scale)
    gn = np.array([np.linalg.norm(d[q] * np.linalg.lstsq(A[q], b[q], rcond=None)[0]) for q in range(count)])
    frac = np.array([T.FRACS[q % len(T.FRACS)] for q in range(count)])
    delta = frac * gn
    out = _gels_trust(plan, A, b, delta, d, rtol=rtol)
    tag = f"{'fused' if fused else 'composed'} {m}x{n}"
    _check_rule(tag, out, delta, d, rtol, frac if m > n else None)           # (a square member has no residual to speak of; f is only a scale)
    # dA, dtau and dB come back as qr_gels_damped_batched_dev leaves them
    dm = _fused(plan, A, b[:, :, None], d, np.where(out["lam"] > 0, out["lam"], 1.0)[:, None])
    assert np.array_equal(dm["F"], out["F"]) and np.array_equal(dm["tau"], out["tau"]) and np.array_equal(dm["QtB"][:, :, 0], out["Qtb"])
    # X, xnorm and resid are bitwise qr_gels_damped_batched_dev's at the lambda returned; and the search on the factors it left is the
    # same search, bit for bit
    rss = (out["Qtb"][:, n:] ** 2).sum(axis=1)
    pos = out["lam"] > 0
    assert np.array_equal(dm["X"][pos, 0, :, 0], out["X"][pos]) and np.array_equal(dm["xnorm"][pos, 0, 0], out["xnorm"][pos])
    assert np.array_equal(dm["resid"][pos, 0, 0], out["resid"][pos])
    if fused:
        again = _trust(plan, out["F"][:, :n], out["Qtb"][:, :n], delta, d, None, rtol=rtol)
        _same(out, again, ("X", "lam", "xnorm", "iter", "status", "info"))  # (resid: the tail sum is the factoring call's own)
        g = _gels(plan, A, b[:, :, None])
        acc = out["status"] == 1
        assert acc.any() and np.array_equal(g["B"][acc, :n, 0], out["X"][acc])     # check 3: the accepted step is qr_gels_batched_dev's
    else:
        dR, dZ = Strided(m, n, count, out["F"]), Strided(m, 1, count, out["Qtb"][:, :, None])
        o = Out(n, count)
        dD = Strided(n, 1, count, d[:, :, None])
        plan.trust_batched(dR.ptr, n, dR.ld, dR.stride, dZ.ptr, dZ.ld, dZ.stride, _dev(delta), 1, o.X.ptr, o.X.ld, o.X.stride, o.lam, o.info,
                           count, drss=_dev(rss), dD=dD.ptr, strideD=dD.stride, rtol=rtol, **o.kw())
        plan.sync()
        _same(out, o.collect(), ("X", "lam", "xnorm", "iter", "status", "info"))


# ------------------------------------------------------------------------------------------------
# rank-deficient members
# ------------------------------------------------------------------------------------------------
def test_pivoted_factors_of_rank_deficient_members(plan):
    b, m, n, r = 5, 64, 28, 5
    A = np.stack([T.D.U(900 + q, m, r) @ T.D.U(950 + q, r, n) for q in range(b)])
    bb, d = T.D.U(990, b, m), 0.5 + 1.5 * np.random.default_rng(991).random((b, n))
    dA, dtau, dj = Strided(m, n, b, A), Strided(n, 1, b), Strided(n, 1, b, dtype=np.int32)
    plan.geqp3_batched(dA.ptr, m, n, dA.ld, dA.stride, dj.ptr, dj.stride, dtau.ptr, dtau.stride, b)
    dB = Strided(m, 1, b, bb[:, :, None])
    plan.ormqr_batched("T", dA.ptr, m, n, dA.ld, dA.stride, dtau.ptr, dtau.stride, dB.ptr, 1, dB.ld, dB.stride, b)
    plan.sync()
    F, Qtb, jp = dA.get(), dB.get()[:, :, 0], dj.get()[:, :, 0]
    R, z, rss = F[:, :n], Qtb[:, :n], (Qtb[:, n:] ** 2).sum(axis=1)
    # the scale of the radii: the minimum-norm solution's |D x| (the Gauss-Newton step of factors of numerical rank 5 is far larger)
    base = np.array([np.linalg.norm(d[q] * np.linalg.lstsq(A[q], bb[q], rcond=None)[0]) for q in range(b)])
    # (fractions well below 1: as Delta approaches the minimum-norm |D x| the lambda sought goes to 0 on a singular R, the limit in
    # which lmpar's Newton steps slow down; the float64 restatement needs at most 8 of the 10 iterations on these)
    for rtol in T.RTOLS:
        delta = np.array([0.5, 1e-2, 0.1, 1e-6, 0.3]) * base
        out = _trust(plan, R, z, delta, d, rss, jpvt=jp, rtol=rtol)
        _check_rule("pivoted rank 5", out, delta, d, rtol, None, full_rank=False)
        assert np.all(out["lam"] > 0) and np.all(out["xnorm"] <= (1 + rtol) * delta)
        _check_is_damped(plan, out, R, z, d, rss, jpvt=jp)


@pytest.mark.parametrize("n,zero", [(12, 9), (40, 33)])
def test_exactly_zero_trailing_columns(plan, n, zero):
    p = _problem(n + 3, n, 5)
    R = p["R"].copy()
    R[:, :, zero:] = 0.0                                      # nsing = zero: the Gauss-Newton step solves the leading block
    gn = np.array([T.gauss_newton_dxnorm(R[q][:zero, :zero], p["z"][q][:zero], p["d"][q][:zero]) for q in range(5)])
    delta = p["frac"] * gn
    for rtol in T.RTOLS:
        out = _trust(plan, R, p["z"], delta, p["d"], p["rss"], rtol=rtol)
        _check_rule(f"zero columns n={n}", out, delta, p["d"], rtol, None, full_rank=False)
        assert np.all(out["xnorm"] <= (1 + rtol) * delta)
        assert np.all(out["X"][out["status"] == 1][:, zero:] == 0.0) and np.all(out["status"][:2] == 1)
        pos = out["lam"] > 0
        assert pos.sum() == 3
        dm = _damped(plan, R, p["z"][:, :, None], p["d"], np.where(pos, out["lam"], 1.0)[:, None], p["rss"][:, None])
        assert np.all(dm["info"] == 0) and np.array_equal(dm["X"][pos, 0, :, 0], out["X"][pos])    # with lambda > 0 there is no info word
        # a zero column with d_c = 0: nothing damps it, info c + 1 as in the damped call; the neighbours are unaffected
        d0 = p["d"].copy()
        d0[2, zero + 1] = 0.0
        bad = _trust(plan, R, p["z"], delta, d0, p["rss"], rtol=rtol)
        info = np.zeros(5, dtype=int)
        info[2] = zero + 2
        assert np.array_equal(bad["info"], info) and np.all(bad["X"][2] == SENTINEL) and bad["lam"][2] == SENTINEL
        _same(bad, out, members=[0, 1, 3, 4])


# ------------------------------------------------------------------------------------------------
# the accumulator
# ------------------------------------------------------------------------------------------------
def test_accumulator_call_is_the_call_on_its_state(qr, plan):
    b, n, m = 5, 8, 40
    A, bb, d = T.batch(m, n, b)
    acc = qr.LsAccumulatorBatched(plan, n, 1, b)
    try:
        dA, dB = Strided(m, n, b, A), Strided(m, 1, b, bb[:, :, None])
        acc.push(dA.ptr, m, dA.ld, dA.stride, dB.ptr, dB.ld, dB.stride)
        plan.sync()
        s0 = [np.array(x) for x in acc.factor_host()]
        R, Z, rss = s0[0], s0[1], s0[2]
        z = Z[:, :, 0]
        delta = np.array([T.FRACS[q % 5] * T.gauss_newton_dxnorm(np.triu(R[q]), z[q], d[q]) for q in range(b)])
        o = Out(n, b)
        dD = Strided(n, 1, b, d[:, :, None])
        acc.solve_trust(_dev(delta), 1, o.X.ptr, o.X.ld, o.X.stride, o.lam, o.info, dD=dD.ptr, strideD=dD.stride, rtol=1e-3, **o.kw())
        plan.sync()
        out = o.collect()
        assert all(np.array_equal(x, y) for x, y in zip(s0, [np.array(x) for x in acc.factor_host()])), "the state is untouched"
        _check_rule("accumulator", out, delta, d, 1e-3, np.array(T.FRACS))
        _same(out, _trust(plan, R, z, delta, d, rss[:, 0], rtol=1e-3))
    finally:
        acc.close()


# ------------------------------------------------------------------------------------------------
# wide members, D = I
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(6, 7), (1, 2), (8, 64), (33, 100)])
def test_wide_members(plan, m, n):
    A, b, _ = T.batch(m, n, 5, with_d=False)
    gn = np.array([np.linalg.norm(np.linalg.lstsq(A[q], b[q], rcond=None)[0]) for q in range(5)])     # the minimum-norm solution
    frac = np.array(T.FRACS)
    delta = frac * gn
    for rtol in T.RTOLS:
        out = _wide_trust(plan, A, b, delta, rtol=rtol)
        assert np.all(out["info"] == 0)
        pos = out["lam"] > 0
        assert np.array_equal(pos, frac < 1) and np.all(out["status"][~pos] == 1) and np.all(out["status"][pos] == 0)
        print(f"ITER wide {m}x{n} rtol {rtol}: iterations {out['iter'].tolist()}")
        # check 2: bitwise qr_gels_damped_wide_batched_dev's at the lambda returned
        dm = _wide(plan, A, b[:, :, None], np.where(pos, out["lam"], 1.0)[:, None])
        assert np.array_equal(dm["X"][pos, 0, :, 0], out["X"][pos]) and np.array_equal(dm["xnorm"][pos, 0, 0], out["xnorm"][pos])
        assert np.array_equal(dm["resid"][pos, 0, 0], out["resid"][pos])
        for q in range(5):
            x = out["X"][q]
            assert T.meets_rule(out["xnorm"][q], out["lam"][q], delta[q], rtol)
            # |x| = |y| up to the rounding of Q: n eps (the orthogonality cap of the minimum-norm tests), and the norm's own
            xl = float(H.norm(H.arr(x)))
            slack = rtol * delta[q] + (n * H.EPS + T.norm_slack(n)) * xl
            assert (xl - delta[q] <= slack) if out["lam"][q] == 0 else (abs(xl - delta[q]) <= slack)
            # x lies in the row space of A.  Measured against an orthonormal basis of it from a float64 Householder QR of A^T: that basis
            # and the kernel's are each the exact basis of a matrix within n eps |A| of A^T, whose range is turned by at most
            # kappa(A) n eps; two such angles, and a factor 2 for the constants of the two factorisations: 4 n kappa(A) eps |x|
            Q = np.linalg.qr(A[q].T)[0]
            assert np.linalg.norm(x - Q @ (Q.T @ x)) <= 4 * n * np.linalg.cond(A[q]) * H.EPS * np.linalg.norm(x)


# ------------------------------------------------------------------------------------------------
# host pointers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(20, 6), (6, 20)])
def test_host_twin(qr, m, n):
    A, b, d = T.batch(m, n, 5, with_d=m >= n)
    x0 = [np.linalg.lstsq(A[q], b[q], rcond=None)[0] for q in range(5)]
    delta = np.array(T.FRACS) * np.array([np.linalg.norm((1.0 if d is None else d[q]) * x0[q]) for q in range(5)])
    X, lam, xn, rs, it, st, info = qr.lstsq_trust_batched(A, b, delta, D=d, rtol=1e-3)
    assert np.all(info == 0) and np.all(it <= T.MAXIT) and np.all((st == 1) == (lam == 0)) and np.array_equal(st[:2], [1, 1])
    for q in range(5):
        assert T.meets_rule(xn[q], lam[q], delta[q], 1e-3)
        dx = (1.0 if d is None else d[q]) * X[q]
        assert abs(np.linalg.norm(dx) - xn[q]) <= 4 * (n + 4) * H.EPS * xn[q]
        assert abs(np.linalg.norm(A[q] @ X[q] - b[q]) - rs[q]) <= 1e-8 * max(rs[q], np.linalg.norm(b[q]))
    delta[1] = -1.0
    X, lam, xn, rs, it, st, info = qr.lstsq_trust_batched(A, b, delta, D=d)
    assert info.tolist() == [0, -1, 0, 0, 0]
