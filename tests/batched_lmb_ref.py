"""A numpy restatement of the bounded batched Levenberg-Marquardt solver (mi355x_qr.h section 8n; kernels: csrc/qr_batched_lm.hip) for one
member, on top of batched_lm_ref.Member, with the bounded test problems (helper module, no fixtures, no GPU).

BMember adds the three rules to Member: P (the peg, on the unfactored J and f, the sum in the kernel's order: lane l takes rows l,
l + 64, .. ascending by fma, then the butterfly over the 64 lanes), S (the step cut to the box, after Member.step_factors has run rules a
to i on the search's step) and U (Member.update, and while clipped is set the status formed again without the two tests on the
reductions).  Nothing of Member is restated: with every bound infinite a BMember is a Member bit for bit.  dtype float64 or longdouble.

margin: the smallest |g_j| / (m eps |J_j| |f|) over the peg decisions taken (inf if none): tests/test_batched_lmb_ref.py demands more than
64 of the longdouble instance on every member, so that no decision of the device sits within rounding of a sign change.
"""
from fractions import Fraction

import numpy as np

import batched_lm_ref as L
import hp_ref as H

LD = H.LD
EPS = H.EPS
INF = float("inf")
EXTRA = ("lo", "hi", "peg", "alpha", "clipped")


def _fma(a, b, c):
    """fma(a, b, c) of float64 values, correctly rounded"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def peg_sum(col, f, dtype=np.float64):
    """sum_i col_i f_i as blmb_peg_kernel forms it"""
    m = len(col)
    acc = H.arr(np.zeros(64), dtype)
    for i in range(m):
        l = i % 64
        acc[l] = _fma(col[i], f[i], acc[l]) if dtype == np.float64 else col[i] * f[i] + acc[l]
    idx = np.arange(64)
    o = 32
    while o:
        acc = acc + acc[idx ^ o]
        o >>= 1
    return acc[0]


class BMember(L.Member):
    """the state of one member and the two device calls on it, with lo <= x <= hi"""

    def __init__(self, x0, lo=None, hi=None, dtype=np.float64, D0=None, **options):
        super().__init__(x0, dtype, D0, **options)
        n = self.n
        self.lo = H.arr(np.broadcast_to(-INF if lo is None else np.asarray(lo, dtype=np.float64), (n,)).copy(), dtype)
        self.hi = H.arr(np.broadcast_to(INF if hi is None else np.asarray(hi, dtype=np.float64), (n,)).copy(), dtype)
        self.peg = np.zeros(n, dtype=np.int64)
        self.alpha, self.clipped = self.c(1.0), 0
        self.margin = INF
        if not np.all(self.lo <= self.hi) or np.any(self.x < self.lo) or np.any(self.x > self.hi):
            self.info = -2

    def step(self, J, f):
        """qr_lmb_batched_step_dev: the peg, geqp3 of J with the held columns cleared, Q^T f, the step"""
        if not self.running():
            return
        n = self.n
        J, f = H.arr(J, self.dtype).copy(), H.arr(f, self.dtype)
        m = J.shape[0]
        for j in range(n):
            atlo, athi = self.x[j] == self.lo[j], self.x[j] == self.hi[j]
            pg = 0
            if atlo or athi:
                g = peg_sum(J[:, j], f, self.dtype)
                scale = m * EPS * float(H.norm(J[:, j])) * float(H.norm(f))
                self.margin = min(self.margin, abs(float(g)) / scale if scale else 0.0)
                if atlo and g > 0:
                    pg = -1
                elif athi and g < 0:
                    pg = 1
                if pg:
                    J[:, j] = 0
            self.peg[j] = pg
        F, tau, jp = H.qrp(J, self.dtype)
        y = H.apply_q(F, tau, f, "T", self.dtype)
        self.step_factors(np.triu(F[:n]), y, jp)

    def step_factors(self, R, zall, jpvt=None, rss=0.0):
        if not self.running():
            return
        self.p = None
        super().step_factors(R, zall, jpvt, rss)              # rules a to i on the search's step
        if self.p is None or not self.running():
            return
        n, c, root = self.n, self.c, self.root
        x, lo, hi = self.x, self.lo, self.hi
        s = -self.p
        hold = (self.peg != 0) | ((x <= lo) & (s < 0)) | ((x >= hi) & (s > 0))
        zeroed = bool(np.any(hold & (s != 0)))
        s = np.where(hold, c(0.0), s)
        r = H.arr(np.full(n, INF), self.dtype)
        bound = H.arr(np.zeros(n), self.dtype)
        for j in range(n):
            if s[j] != 0:
                t = x[j] + s[j]
                if t < lo[j]:
                    r[j], bound[j] = (lo[j] - x[j]) / s[j], lo[j]
                elif t > hi[j]:
                    r[j], bound[j] = (hi[j] - x[j]) / s[j], hi[j]
        alpha = min(c(1.0), r.min())
        plain = (not zeroed) and alpha == 1
        pt = -(alpha * s)
        xt = x - pt
        xt = np.where(xt < lo, lo, xt)
        xt = np.where(xt > hi, hi, xt)
        xt = np.where(r == alpha, bound, xt)
        self.xtrial, self.alpha, self.clipped = xt, alpha, int(alpha < 1)
        if plain:
            return
        R = H.arr(np.triu(np.asarray(R)[:n, :n]), self.dtype)
        z = H.arr(zall, self.dtype)[:n]
        jp = np.arange(n) if jpvt is None else np.asarray(jpvt)
        zs = z / self.fnorm
        gk = np.array([(R[:k + 1, k] * zs[:k + 1]).sum() for k in range(n)])
        pp = pt[jp]
        rp = z * 0
        for k in range(n):
            rp = rp + R[:, k] * pp[k]
        temp1 = root((rp * rp).sum()) / self.fnorm
        pg = (pp * gk).sum() / self.fnorm
        self.prered = max(c(0.0), c(2.0) * pg - temp1 * temp1)
        self.dirder = -pg
        self.p = pt

    def update(self, ftrial):
        """qr_lmb_batched_update_dev"""
        if not self.running():
            return
        super().update(ftrial)
        if not self.clipped:
            return
        o, eps = self.o, self.c(EPS)                           # the status again, without tests 1 and 6
        st = 0
        if self.delta <= self.c(o["xtol"]) * self.xnorm:
            st = 2
        if st == 0:
            if self.nfev >= o["maxfev"]:
                st = 5
            if self.delta <= eps * self.xnorm:
                st = 7
            if self.gnorm <= eps:
                st = 8
        self.status = st


def solve(problem, x0, data, lo, hi, dtype=np.float64, D0=None, **options):
    """the whole solve of one member: the BMember at its end"""
    mem = BMember(x0, lo, hi, dtype, D0, **options)
    dat = None if data is None else H.arr(data, dtype)
    while mem.running():
        mem.step(problem.jac(np, mem.x, dat), problem.f(np, mem.x, dat))
        if mem.running():
            mem.update(problem.f(np, mem.xtrial, dat))
    return mem


# ----------------------------------------------------------------------------------------------------------------------------------
# the bounded problems: members(count, first=0) -> (x0, data, lo, hi), member q seeded by first + q alone
# ----------------------------------------------------------------------------------------------------------------------------------
class ExpDecayB(L.ExpDecay):
    """ExpDecay(16) with the rate bounded above by 0.8 of the planted rate: the bound cuts off the free minimiser.  a, c >= 0.  gtol =
    1e-8: the run ends by the projected gradient (1e-15 at the minimiser), not by a last trial step whose reductions are rounding"""
    options = dict(gtol=1e-8)

    def __init__(self):
        super().__init__(16)
        self.name, self.batch = "expdecay_b", 9

    def members(self, count, first=0):
        x0, data, lo, hi = [], [], [], []
        for q in range(first, first + count):
            rng = np.random.default_rng(5100 + q)
            xs = np.array([1.0 + rng.random(), 0.5 + rng.random(), 0.25 + 0.5 * rng.random()])
            h = np.array([INF, 0.8 * xs[1], INF])
            s = xs * (1.0 + 0.2 * np.sign(rng.random(3) - 0.5))
            s[1] = 0.5 * h[1]
            x0.append(s), data.append(self.model(np, xs)), lo.append(np.zeros(3)), hi.append(h)
        return np.stack(x0), np.stack(data), np.stack(lo), np.stack(hi)


class GaussPeakB(L.GaussPeak):
    """GaussPeak with a floor on the width 1.2 times the planted width; the amplitude >= 0"""
    options = {}

    def __init__(self):
        super().__init__()
        self.name, self.batch = "gausspeak_b", 9

    def members(self, count, first=0):
        x0, data, lo, hi = [], [], [], []
        for q in range(first, first + count):
            rng = np.random.default_rng(5200 + q)
            xs = np.array([1.0 + rng.random(), 0.6 * (rng.random() - 0.5), 0.7 + 0.5 * rng.random(), 0.2 + 0.3 * rng.random()])
            l = np.array([0.0, -INF, 1.2 * xs[2], -INF])
            sg = np.sign(rng.random(4) - 0.5)
            s = xs * (1.0 + 0.1 * sg)
            s[1] = xs[1] + 0.1 * sg[1]
            s[2] = 1.5 * l[2]
            x0.append(s), data.append(self.model(np, xs)), lo.append(l), hi.append(np.full(4, INF))
        return np.stack(x0), np.stack(data), np.stack(lo), np.stack(hi)


class RosenbrockB(L.Rosenbrock):
    """Rosenbrock with x_0 <= hi_0 < 1 (hi_0 = 0.5 + q / 50 for member q)"""
    options = {}
    name, batch = "rosenbrock_b", 5

    def members(self, count, first=0):
        x0 = np.stack([np.array([-1.2, 1.0]) * (1.0 + q / 4.0) for q in range(first, first + count)])
        hi = np.stack([np.array([0.5 + (q % 20) / 50.0, INF]) for q in range(first, first + count)])
        return x0, None, np.full((count, 2), -INF), hi


class LinearBox(L.Problem):
    """f = A x - b with A (m x n) and b seeded per member (the data carries A column-major, then b), a box around 0 that cuts off about
    half of the free minimiser's entries, and for n >= 2 the last parameter fixed by lo = hi.  gtol = 1e-8 for the reason
    batched_lm_ref.LinearFullRank has it: at the minimiser one more trial step is rounding, and float64 and longdouble decide it differently"""
    options = dict(gtol=1e-8)

    def __init__(self, m, n, batch=None, fix=True):
        self.name, self.m, self.n, self.batch = f"linbox{m}x{n}" if fix else f"linboxfree{m}x{n}", m, n, L.linear_batch(m, n) if batch is None else batch
        self.fix = fix

    def split(self, xp, data):
        m, n = self.m, self.n
        A = data[..., :m * n].reshape(tuple(data.shape[:-1]) + (n, m))
        return (xp.swapaxes(A, -1, -2)), data[..., m * n:]

    def f(self, xp, x, data):
        """(the columns added one by one, ascending: a library reduction may choose its order by the size of the whole batch, and a
        member's f must not depend on its neighbours)"""
        A, b = self.split(xp, data)
        acc = A[..., 0] * x[..., 0:1]
        for j in range(1, self.n):
            acc = acc + A[..., j] * x[..., j:j + 1]
        return acc - b

    def jac(self, xp, x, data):
        A, _ = self.split(xp, data)
        return A + x[..., None, :1] * 0

    def members(self, count, first=0):
        m, n = self.m, self.n
        x0, data, lo, hi = [], [], [], []
        for q in range(first, first + count):
            rng = np.random.default_rng(5300 + 1000 * m + 10 * n + q)
            A = rng.uniform(-1.0, 1.0, (m, n))
            b = A @ rng.uniform(-1.0, 1.0, n) + 0.1 * rng.standard_normal(m)
            l, h = -0.5 - 0.2 * rng.random(n), 0.5 + 0.2 * rng.random(n)
            if n >= 2 and self.fix:
                l[n - 1] = h[n - 1] = 0.25
            s = l + (h - l) * rng.uniform(0.2, 0.8, n)
            x0.append(s), data.append(np.concatenate([A.T.ravel(), b])), lo.append(l), hi.append(h)
        return np.stack(x0), np.stack(data), np.stack(lo), np.stack(hi)


# the shapes of the device tests: both routes, each wave width and its edge, one and several row passes of the peg, the largest
SHAPES = ((1, 1), (3, 1), (16, 3), (16, 7), (24, 8), (65, 16), (64, 31), (512, 31), (100, 33), (256, 63))
KINDS = {p.name: p for p in (ExpDecayB(), GaussPeakB(), RosenbrockB(), LinearBox(24, 6, 9))}
PROBLEMS = dict(KINDS)
PROBLEMS.update({p.name: p for p in (LinearBox(m, n) for m, n in SHAPES)})
# no parameter fixed, so no column is held at the first step: a column held there gets MINPACK's D_j = 1 for a zero column, which does not
# follow a scaling of (f, J), and the scaling test of the workgroup route needs members without one
PROBLEMS["linboxfree100x33"] = LinearBox(100, 33, fix=False)
MARGIN = 64.0
# |x - x_trf| / |x_trf|: the worst over the 80 members of the four kinds, measured with the restatement (gausspeak_b, which ends by ftol at
# |g| ~ 1e-4 of |J||f|; the other kinds stay below 5e-9), times 10, because the two algorithms stop by different rules
TRF_WORST, TRF_CAP = 4.98e-7, 4.98e-6
# the linear members against lsq_linear(bvls), which is exact to rounding: measured 2.64e-15 (linbox64x31), times 10
BVLS_WORST, BVLS_CAP = 2.64e-15, 2.64e-14


def good_members(problem, count, dtype_check=LD):
    """the first `count` members (seeds ascending) whose every peg decision in the longdouble instance keeps MARGIN: (x0, data, lo, hi,
    the float64 members, the longdouble members)"""
    keep, r64, rld = [], [], []
    q = 0
    while len(keep) < count:
        x0, data, lo, hi = problem.members(1, q)
        d = None if data is None else data[0]
        ml = solve(problem, x0[0], d, lo[0], hi[0], dtype_check, **problem.options)
        if ml.margin > MARGIN:
            keep.append((x0[0], d, lo[0], hi[0]))
            rld.append(ml)
            r64.append(solve(problem, x0[0], d, lo[0], hi[0], np.float64, **problem.options))
        q += 1
        assert q < 4 * count + 8, "too many members within rounding of a peg decision"
    x0 = np.stack([k[0] for k in keep])
    data = None if keep[0][1] is None else np.stack([k[1] for k in keep])
    return x0, data, np.stack([k[2] for k in keep]), np.stack([k[3] for k in keep]), r64, rld
