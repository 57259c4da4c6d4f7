"""A numpy restatement of the batched Levenberg-Marquardt solver (mi355x_qr.h section 8m; kernels: csrc/qr_batched_lm.hip) for one member,
with the test problems (helper module, no fixtures, no GPU).

Member is MINPACK lmder's outer loop split as the device calls split it: step(J, f) from the Jacobian and f at x (hp_ref.qrp is dlaqp2,
hp_ref.apply_q forms Q^T f; step_factors is the one new launch on factors that exist), update(ftrial) from f at xtrial.  Every rule is
written in the order the kernels evaluate it; dtype float64 or longdouble, like hp_ref.py.  search() is batched_trust_ref.lmpar with the
start given as par (not as a lambda to be squared) and par returned: the eliminations are batched_damped_ref.solve and .step, as there.

The two places where the solver differs from MINPACK by rounding are restated as the kernels have them: fnorm is taken from Q^T f (all m
rows) at every step, and acnorm from the columns of R.

The problems are written once over an array namespace (numpy of either dtype, or torch on the device): f(xp, x, data) maps x (..., n)
to (..., m), jac to (..., m, n).  Each has the start More, Garbow and Hillstrom give (member q: the start times 1 + q / 4 where a batch
needs different members), or a planted x with a stated perturbation.
"""
import numpy as np

import batched_damped_ref as DR
import batched_trust_ref as T
import hp_ref as H

LD = H.LD
EPS = H.EPS
TINY = T.TINY
DEFAULTS = dict(ftol=float(np.sqrt(EPS)), xtol=float(np.sqrt(EPS)), gtol=0.0, factor=100.0, par_rtol=0.1, maxfev=0, mode=1, par_maxit=10)
SCALARS = ("delta", "par", "fnorm", "xnorm", "pnorm", "gnorm", "prered", "dirder")
COUNTERS = ("iter", "nfev", "njev", "accepted", "status", "info", "par_status")


def search(R, z, delta, d, jpvt, par0, rtol, maxit, dtype=np.float64):
    """batched_trust_ref.lmpar from factors with the starting par given: dict(X in the caller's order, par, xnorm, iter, status, info)"""
    fail = lambda info: dict(X=None, par=None, xnorm=None, iter=None, status=None, info=info)
    if not (np.isfinite(float(delta)) and delta > 0):
        return fail(-1)
    R0, z0 = H.arr(np.triu(np.asarray(R)), dtype), H.arr(z, dtype)
    n = R0.shape[0]
    jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
    dd = H.arr(np.asarray(d)[jp], dtype)
    delta, rtol = H.arr(delta, dtype), H.arr(rtol, dtype)
    nrm = lambda v: H._root((v * v).sum(), dtype)

    def finish(x, par, xnorm, it, status):
        X = x * 0
        X[jp] = x
        return dict(X=X, par=par, xnorm=xnorm, iter=it, status=status, info=0)

    nsing = n
    for i in range(n):
        if R0[i, i] == 0:
            nsing = i
            break
    x = z0 * 0
    if nsing:
        x[:nsing] = H.solve_r(R0[:nsing, :nsing], z0[:nsing], dtype)
    dxnorm = nrm(dd * x)
    fp = dxnorm - delta
    if fp <= rtol * delta:
        return finish(x, H.arr(0.0, dtype), dxnorm, 0, 1)
    parl = H.arr(0.0, dtype)
    if nsing == n:
        w = nrm(H.solve_rt(R0, dd * ((dd * x) / dxnorm), dtype))
        parl = ((fp / delta) / w) / w
    g = np.array([(R0[:j + 1, j] * z0[:j + 1]).sum() / dd[j] if dd[j] != 0 else 0 * dd[j] for j in range(n)])
    gnorm = T.gradient_norm(g, dtype)
    paru = gnorm / delta
    if paru == 0:
        paru = H.arr(TINY, dtype) / min(delta, H.arr(0.1, dtype))
    par = min(max(H.arr(par0, dtype), parl), paru)
    if par == 0:
        par = gnorm / dxnorm
    it = 0
    while True:
        it += 1
        if par == 0:
            par = max(H.arr(TINY, dtype), H.arr(0.001, dtype) * paru)
        lam = H._root(par, dtype)
        X, xn, _, info = DR.solve(R0, z0[:, None], lam, dd, None, None, False, dtype)
        if info:
            return fail(info)
        x, dxnorm = X[:, 0], xn[0]
        prev, fp = fp, dxnorm - delta
        if abs(fp) <= rtol * delta:
            return finish(x, par, dxnorm, it, 0)
        if parl == 0 and fp <= prev and prev < 0:
            return finish(x, par, dxnorm, it, 2)
        if it >= maxit:
            return finish(x, par, dxnorm, it, 3)
        Rt, _ = DR.step(R0, z0[:, None], lam * dd, dtype)
        w = nrm(H.solve_rt(Rt, dd * ((dd * x) / dxnorm), dtype))
        parc = ((fp / delta) / w) / w
        if fp > 0:
            parl = max(parl, par)
        if fp < 0:
            paru = min(paru, par)
        par = max(parl, par + parc)


class Member:
    """the state of one member and the two device calls on it"""

    def __init__(self, x0, dtype=np.float64, D0=None, **options):
        o = dict(DEFAULTS)
        o.update(options)
        self.dtype = dtype
        self.n = n = len(x0)
        if not o["maxfev"]:
            o["maxfev"] = 100 * (n + 1)
        self.o = o
        self.x = H.arr(x0, dtype)
        self.xtrial = self.x.copy()
        self.D = H.arr(np.ones(n) if o["mode"] != 2 else D0, dtype)
        for k in SCALARS:
            setattr(self, k, H.arr(0.0, dtype)[()])
        self.iter, self.nfev, self.njev, self.accepted, self.status, self.info, self.par_status = 1, 1, 0, 0, 0, 0, 0
        self.kappa = 0.0              # the largest condition number of J D^-1 met (inf for a rank-deficient one)
        self.p = None                 # the last step, in the caller's order

    def running(self):
        return self.status == 0 and self.info == 0

    def c(self, v):
        return H.arr(v, self.dtype)[()]

    def root(self, v):
        return H._root(v, self.dtype)

    def step(self, J, f):
        """qr_lm_batched_step_dev: geqp3 of J, Q^T f, the step"""
        if not self.running():
            return
        n = self.n
        F, tau, jp = H.qrp(J, self.dtype)
        y = H.apply_q(F, tau, f, "T", self.dtype)
        self.step_factors(np.triu(F[:n]), y, jp)

    def step_factors(self, R, zall, jpvt=None, rss=0.0):
        """qr_lm_step_batched_dev: R (n x n), zall (the top zrows >= n rows of Q^T f), rss (the squares of the rows that are not there)"""
        if not self.running():
            return
        n, o, c, root = self.n, self.o, self.c, self.root
        R = H.arr(np.triu(np.asarray(R)[:n, :n]), self.dtype)
        zall = H.arr(zall, self.dtype)
        z, tail = zall[:n], zall[n:]
        jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
        fnorm = root((z * z).sum() + ((tail * tail).sum() + c(rss)))
        acn = np.array([root((R[:k + 1, k] * R[:k + 1, k]).sum()) for k in range(n)])
        if self.njev == 0:
            if o["mode"] != 2:
                for k in range(n):
                    self.D[jp[k]] = acn[k] if acn[k] != 0 else c(1.0)
            elif not all(self.D > 0):
                self.info = -1
                return
            dx = self.D * self.x
            self.xnorm = root((dx * dx).sum())
            self.delta = c(o["factor"]) * self.xnorm
            if self.delta == 0:
                self.delta = c(o["factor"])
        gnorm = c(0.0)
        if fnorm != 0:
            zs = z / fnorm
            for k in range(n):
                if acn[k] != 0:
                    gnorm = max(gnorm, abs((R[:k + 1, k] * zs[:k + 1]).sum() / acn[k]))
        done = gnorm <= o["gtol"]
        if not done and o["mode"] != 2:
            for k in range(n):
                self.D[jp[k]] = max(self.D[jp[k]], acn[k])
        self.fnorm, self.gnorm = fnorm, gnorm
        self.njev += 1
        if done:
            self.status = 4
            return
        if not (np.isfinite(float(self.delta)) and self.delta > 0):
            self.info, self.status = -1, -1
            return
        s = np.linalg.svd(np.asarray(R, dtype=np.float64) / np.asarray(self.D, dtype=np.float64)[jp][None, :], compute_uv=False)
        self.kappa = max(self.kappa, float(s[0] / s[-1]) if s[-1] > 0 else np.inf)
        res = search(R, z, self.delta, self.D, jp, self.par, o["par_rtol"], o["par_maxit"], self.dtype)
        if res["info"]:
            self.info, self.status = res["info"], -1
            return
        self.p, self.par, self.pnorm, self.par_status = res["X"], res["par"], res["xnorm"], res["status"]
        self.xtrial = self.x - self.p
        if self.iter == 1:
            self.delta = min(self.delta, self.pnorm)
        pp = self.p[jp]
        rp = z * 0
        for k in range(n):                                    # R P^T p, the columns ascending
            rp = rp + R[:, k] * pp[k]
        temp1 = root((rp * rp).sum()) / fnorm
        temp2 = (root(self.par) * self.pnorm) / fnorm
        t1, t2 = temp1 * temp1, temp2 * temp2
        self.prered = t1 + t2 / c(0.5)
        self.dirder = -(t1 + t2)

    def update(self, ftrial):
        """qr_lm_batched_update_dev"""
        if not self.running():
            return
        o, c, root = self.o, self.c, self.root
        ft = H.arr(ftrial, self.dtype)
        fnorm1 = root((ft * ft).sum())
        eps = c(EPS)
        finite = bool(np.isfinite(float(fnorm1)))
        worse = (not finite) or c(0.1) * fnorm1 >= self.fnorm
        actred = c(-1.0)
        if finite and c(0.1) * fnorm1 < self.fnorm:
            fr = fnorm1 / self.fnorm
            actred = c(1.0) - fr * fr
        ratio = actred / self.prered if self.prered != 0 else c(0.0)
        if ratio <= 0.25:
            temp = c(0.5) if actred >= 0 else c(0.5) * self.dirder / (self.dirder + c(0.5) * actred)
            if worse or temp < c(0.1):
                temp = c(0.1)
            self.delta = temp * min(self.delta, self.pnorm / c(0.1))
            self.par = self.par / temp
        elif self.par == 0 or ratio >= 0.75:
            self.delta = self.pnorm / c(0.5)
            self.par = c(0.5) * self.par
        self.accepted = int(ratio >= c(1.0e-4))
        if self.accepted:
            self.x = self.xtrial.copy()
            dx = self.D * self.x
            self.xnorm = root((dx * dx).sum())
            self.fnorm = fnorm1
            self.iter += 1
        self.nfev += 1
        small = c(0.5) * ratio <= 1
        st = 0
        if abs(actred) <= o["ftol"] and self.prered <= o["ftol"] and small:
            st = 1
        if self.delta <= c(o["xtol"]) * self.xnorm:
            st = 3 if st == 1 else 2
        if st == 0:
            if self.nfev >= o["maxfev"]:
                st = 5
            if abs(actred) <= eps and self.prered <= eps and small:
                st = 6
            if self.delta <= eps * self.xnorm:
                st = 7
            if self.gnorm <= eps:
                st = 8
        self.status = st


def solve(problem, x0, data, dtype=np.float64, D0=None, ftrial_hook=None, **options):
    """the whole solve of one member: the Member at its end and the list of (x, accepted, status) after every round.  ftrial_hook(round,
    ftrial) may replace f at the trial point (the NaN / inf tests)"""
    mem = Member(x0, dtype, D0, **options)
    dat = None if data is None else H.arr(data, dtype)
    trace = []
    rounds = 0
    while mem.running():
        mem.step(problem.jac(np, mem.x, dat), problem.f(np, mem.x, dat))
        if mem.running():
            ft = problem.f(np, mem.xtrial, dat)
            if ftrial_hook is not None:
                ft = ftrial_hook(rounds, ft)
            mem.update(ft)
        trace.append((np.array(mem.x, dtype=np.float64), mem.accepted, mem.status))
        rounds += 1
    return mem, trace


# ----------------------------------------------------------------------------------------------------------------------------------
# the problems
# ----------------------------------------------------------------------------------------------------------------------------------
def const(xp, x, values):
    """`values` as an array of x's namespace, dtype and device"""
    if xp is np:
        return np.asarray(values, dtype=x.dtype)
    return xp.as_tensor(np.asarray(values, dtype=np.float64), dtype=x.dtype, device=x.device)


class Problem:
    name, m, n = "", 0, 0
    planted = False
    options = {}                  # the qr_lm_options fields the problem is run with (the others: the defaults)
    batch = 5                     # the batch size its whole solves run at

    def members(self, count):
        """(x0 (count, n), data (count, m) or None, planted x (count, n) or None)"""
        raise NotImplementedError

    def mgh(self, x0, count):
        x0 = np.asarray(x0, dtype=np.float64)
        return np.stack([x0 * (1.0 + q / 4.0) for q in range(count)]), None, None


class ExpDecay(Problem):
    """y = a exp(-b t) + c on m points of [0, 4]; planted (a, b, c) seeded per member, the start the planted x times 1 +- 0.2"""
    planted = True

    def __init__(self, m):
        self.name, self.m, self.n, self.batch = f"expdecay{m}", m, 3, 9 if m == 16 else 5
        self.t = np.linspace(0.0, 4.0, m)

    def model(self, xp, x):
        t = const(xp, x, self.t)
        a, b, c = x[..., 0:1], x[..., 1:2], x[..., 2:3]
        return a * xp.exp(-b * t) + c

    def f(self, xp, x, data):
        return self.model(xp, x) - data

    def jac(self, xp, x, data):
        t = const(xp, x, self.t)
        a, b = x[..., 0:1], x[..., 1:2]
        e = xp.exp(-b * t)
        return xp.stack([e, -a * t * e, e * 0 + 1], -1)

    def members(self, count):
        rng = np.random.default_rng(20240 + self.m)
        xs = np.stack([1.0 + rng.random(count), 0.5 + rng.random(count), 0.25 + 0.5 * rng.random(count)], 1)
        x0 = xs * (1.0 + 0.2 * np.sign(rng.random((count, 3)) - 0.5))
        return x0, self.model(np, xs), xs


class GaussPeak(Problem):
    """y = a exp(-(t - mu)^2 / (2 s^2)) + c on 32 points of [-3, 3]; planted, the start the planted x times 1 +- 0.1 (mu: +- 0.1)"""
    planted = True

    def __init__(self):
        self.name, self.m, self.n, self.batch = "gausspeak", 32, 4, 9
        self.t = np.linspace(-3.0, 3.0, 32)

    def parts(self, xp, x):
        t = const(xp, x, self.t)
        a, mu, s, c = x[..., 0:1], x[..., 1:2], x[..., 2:3], x[..., 3:4]
        u = (t - mu) / s
        return a, s, c, u, xp.exp(-0.5 * u * u)

    def model(self, xp, x):
        a, s, c, u, e = self.parts(xp, x)
        return a * e + c

    def f(self, xp, x, data):
        return self.model(xp, x) - data

    def jac(self, xp, x, data):
        a, s, c, u, e = self.parts(xp, x)
        return xp.stack([e, a * e * u / s, a * e * u * u / s, e * 0 + 1], -1)

    def members(self, count):
        rng = np.random.default_rng(77)
        xs = np.stack([1.0 + rng.random(count), 0.6 * (rng.random(count) - 0.5), 0.7 + 0.5 * rng.random(count), 0.2 + 0.3 * rng.random(count)], 1)
        sg = np.sign(rng.random((count, 4)) - 0.5)
        x0 = xs * (1.0 + 0.1 * sg)
        x0[:, 1] = xs[:, 1] + 0.1 * sg[:, 1]
        return x0, self.model(np, xs), xs


class Rosenbrock(Problem):
    name, m, n, batch = "rosenbrock", 2, 2, 5

    def f(self, xp, x, data):
        return xp.stack([10.0 * (x[..., 1] - x[..., 0] * x[..., 0]), 1.0 - x[..., 0]], -1)

    def jac(self, xp, x, data):
        z, o = x[..., 0] * 0, x[..., 0] * 0 + 1
        return xp.stack([xp.stack([-20.0 * x[..., 0], 10.0 * o], -1), xp.stack([-o, z], -1)], -2)

    def members(self, count):
        return self.mgh([-1.2, 1.0], count)


class PowellSingular(Problem):
    """J is rank-deficient at the solution x = 0, which the iteration approaches linearly; neither ftol nor xtol ever fires.  With gtol = 0
    the run ends some 58 evaluations on at |x| ~ 1e-17 by status 8, on quantities that are rounding (the float64 and the longdouble
    restatement and MINPACK give three different counts for most starts); gtol = 1e-6 ends it at |x| ~ 1e-7, where no decision is"""
    name, m, n, batch = "powell", 4, 4, 9
    options = dict(gtol=1e-6)
    R5, R10 = float(np.sqrt(5.0)), float(np.sqrt(10.0))

    def f(self, xp, x, data):
        x1, x2, x3, x4 = (x[..., i] for i in range(4))
        return xp.stack([x1 + 10.0 * x2, self.R5 * (x3 - x4), (x2 - 2.0 * x3) * (x2 - 2.0 * x3), self.R10 * (x1 - x4) * (x1 - x4)], -1)

    def jac(self, xp, x, data):
        x1, x2, x3, x4 = (x[..., i] for i in range(4))
        z, o = x1 * 0, x1 * 0 + 1
        rows = [[o, 10.0 * o, z, z], [z, z, self.R5 * o, -self.R5 * o], [z, 2.0 * (x2 - 2.0 * x3), -4.0 * (x2 - 2.0 * x3), z],
                [2.0 * self.R10 * (x1 - x4), z, z, -2.0 * self.R10 * (x1 - x4)]]
        return xp.stack([xp.stack(r, -1) for r in rows], -2)

    def members(self, count):
        return self.mgh([3.0, -1.0, 0.0, 1.0], count)


def linear_batch(m, n):
    return 1 if m > 100 else (5 if m * n > 1000 else 9)


class LinearFullRank(Problem):
    """MINPACK's linear function, full rank: f_i = x_i - (2 / m) sum x - 1 (i < n), -(2 / m) sum x - 1 (i >= n); the minimiser is -1.
    The first step lands on it; with gtol = 0 a second trial step follows whose actred and prered are both rounding, and whether it is
    accepted and which of the codes 2 and 3 ends the run differs between MINPACK, float64 and longdouble.  gtol = 1e-8 ends the run at the
    second step by the gradient (1e-15 there): status 4, two evaluations, in all of them"""
    options = dict(gtol=1e-8)

    def __init__(self, m, n):
        self.name, self.m, self.n, self.batch = f"linfull{m}x{n}", m, n, linear_batch(m, n)
        self.J = -2.0 / m * np.ones((m, n))
        self.J[:n] += np.eye(n)

    def f(self, xp, x, data):
        J = const(xp, x, self.J)
        return (J * x[..., None, :]).sum(-1) - 1.0

    def jac(self, xp, x, data):
        J = const(xp, x, self.J)
        return J + x[..., None, :1] * 0

    def members(self, count):
        return self.mgh(np.ones(self.n), count)


class LinearRank1(LinearFullRank):
    """MINPACK's linear function, rank 1: f_i = (i + 1) s - 1, s = sum_j (j + 1) x_j; every x with s = 3 / (2 m + 1) minimises it.
    R(1:, 1:) of its Jacobian is rounding (1e-14 of |J|) and never exactly 0, while Q^T f has entries of order 1 in those rows (the part of
    the constant -1 outside the range of J): the Gauss-Newton step is 1e14 long whatever x is, and every step of lmder fills the radius
    with a direction the rounding of the factorisation decides (MINPACK's own published solution for n = 5, m = 10 has |x| = 295 from a
    start of ones).  No start from which a step is taken gives an x that two implementations share.  The start kept is on the minimising
    plane (member q: s carried by coordinate q mod n alone): with gtol = 1e-8 the first step ends the run by the gradient, status 4, one
    evaluation -- what is exercised is fnorm, acnorm and gnorm on a rank-1 triangle at every shape.  (The search on these triangles is
    covered by the one-step test, bitwise against section 8g on the same factors.)"""

    def __init__(self, m, n):
        self.name, self.m, self.n, self.batch = f"linrank1_{m}x{n}", m, n, linear_batch(m, n)
        self.J = np.outer(np.arange(1.0, m + 1), np.arange(1.0, n + 1))

    def members(self, count):
        x0 = np.zeros((count, self.n))
        for q in range(count):
            j = q % self.n
            x0[q, j] = 3.0 / (2 * self.m + 1) / (j + 1)
        return x0, None, None


class Square1(Problem):
    """(1, 1): f = x^2 - 2"""
    name, m, n, batch = "square1", 1, 1, 1

    def f(self, xp, x, data):
        return x * x - 2.0

    def jac(self, xp, x, data):
        return (2.0 * x)[..., None]

    def members(self, count):
        return self.mgh([3.0], count)


LINEAR_SHAPES = ((5, 3), (64, 31), (65, 4), (64, 32), (100, 33), (256, 63))
# every shape a step kernel is compiled or routed for: the last wave shape, the first workgroup shape by columns, the largest
STEP_SHAPES = ((1, 1), (16, 3)) + LINEAR_SHAPES


def problems():
    out = [ExpDecay(16), ExpDecay(64), GaussPeak(), Rosenbrock(), PowellSingular(), Square1()]
    out += [LinearFullRank(m, n) for m, n in LINEAR_SHAPES]
    out += [LinearRank1(m, n) for m, n in LINEAR_SHAPES]
    return out


PROBLEMS = {p.name: p for p in problems()}
