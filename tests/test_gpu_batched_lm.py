"""-m gpu: the batched Levenberg-Marquardt solver (mi355x_qr.h section 8m), member by member.

Problems, their starts and options, and the restatement: tests/batched_lm_ref.py; tests/test_batched_lm_ref.py shows on the CPU that the
float64 and the longdouble restatement and MINPACK (scipy.optimize.leastsq) take the same decisions on every one of them, which is the
condition under which the whole solves below demand equal counts.

What ties a step to a kernel already verified: xtrial, par, pnorm and par_status are bitwise what qr_trust_batched_dev returns on the same
factors with the kernel's D, the radius of the search and the start.  What ties an update to the rules: every scalar is bitwise the
float64 restatement's on planted tuples that reach every branch.

Figures are printed (-s) before they are asserted; DESIGN.md section 7u tabulates them."""
import functools

import numpy as np
import pytest
import torch

import batched_damped_ref as DR
import batched_lm_ref as L
import hp_ref as H

pytestmark = pytest.mark.gpu

EPS = L.EPS
DOUBLES = ("x", "xtrial", "D") + L.SCALARS
STATE = DOUBLES + L.COUNTERS
MAX_ROUNDS = 700


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


@pytest.fixture(autouse=True)
def _a_device_fault_ends_the_run():
    """nothing more is started on a device that has reported a fault"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported a fault: {e}", returncode=3)


def _dev(v, dtype=torch.float64):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(dtype).cuda()


def _host(st):
    return {k: st[k].cpu().numpy().copy() for k in STATE}


def _same(a, b, keys=STATE, q=None, r=None):
    """bitwise equality of two states (member q of a against member r of b)"""
    for k in keys:
        x, y = (a[k] if q is None else a[k][q]), (b[k] if r is None else b[k][r])
        if not np.array_equal(x, y, equal_nan=True):
            return k
    return None


def _solve(qr, plan, prob, x0, data, trace=False, hook=None, scale=1.0, D0=None, **options):
    """every member through LmBatched with the model in torch on the plan's stream: the final state, and with trace the state after
    every step and after every update"""
    b, n = x0.shape
    m = prob.m
    lm = qr.LmBatched(plan, m, n, b, **options)
    tr = []
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        X0, dat = _dev(x0), _dev(data)
        lm.start(X0, dD0=_dev(D0))
        st = lm.state()
        J = torch.empty((b, n, m), dtype=torch.float64, device="cuda")
        F = torch.empty((b, m), dtype=torch.float64, device="cuda")
        rounds = 0
        while True:
            J.copy_((scale * prob.jac(torch, st["x"], dat)).transpose(1, 2))
            F.copy_(scale * prob.f(torch, st["x"], dat))
            lm.step(J, F)
            if trace:
                tr.append(_host(st))
            Ft = scale * prob.f(torch, st["xtrial"], dat)
            F.copy_(Ft if hook is None else hook(rounds, Ft))
            lm.update(F)
            if trace:
                tr.append(_host(st))
            rounds += 1
            if lm.running() == 0 or rounds >= MAX_ROUNDS:
                break
        out = _host(st)
    lm.close()
    assert rounds < MAX_ROUNDS
    return (out, tr) if trace else out


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the float64 and the longdouble restatement of every member of a problem, once"""
    p = L.PROBLEMS[name]
    x0, data, xs = p.members(p.batch)
    r64 = [L.solve(p, x0[q], None if data is None else data[q], np.float64, **p.options)[0] for q in range(p.batch)]
    rld = [L.solve(p, x0[q], None if data is None else data[q], L.LD, **p.options)[0] for q in range(p.batch)]
    return x0, data, xs, r64, rld


def _rel(a, b):
    a, b = H.arr(a), H.arr(b)
    d, s = float(H.norm(a - b)), float(H.norm(b))
    return d / s if s else d


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. one step, exactly
# ----------------------------------------------------------------------------------------------------------------------------------
def _step_case(m, n, b, kind):
    """J (b, m, n), f (b, m), x (b, n): seeded; kind rank1: every member's J is an outer product"""
    J = np.stack([DR.U(31 * m + n + q, m, n) for q in range(b)])
    if kind == "rank1":
        J = np.stack([np.outer(DR.U(5 * m + q, m), 1.0 + np.arange(n)) for q in range(b)])
    f = np.stack([DR.U(77 * m + n + q, m) for q in range(b)])
    x = np.stack([DR.U(13 * m + n + q, n) for q in range(b)])
    return J, f, x


def _plant_later(st, q):
    """member q as it stands after two accepted steps: a radius, a par that is an exact square, a scaling"""
    st["iter"][q], st["njev"][q], st["nfev"][q] = 3, 2, 3
    st["delta"][q], st["par"][q] = 0.375, 0.0625
    st["D"][q] = 0.5
    st["xnorm"][q] = 1.0


# (m, n, quantity) -> the worst ratio to 4 x the float64 restatement's own distance, where it exceeds 1 (measured on an MI355X; the
# same members stay within 0.38 (m + n) eps of the longdouble restatement: the float64 restatement happens to land closer still)
STEP_EXCEPTIONS = {(16, 3, "prered"): 1.16, (16, 3, "dirder"): 1.16, (16, 3, "fnorm"): 1.02, (5, 3, "gnorm"): 1.78, (5, 3, "fnorm"): 6.97,
                   (64, 31, "prered"): 2.09, (64, 31, "dirder"): 4.05, (100, 33, "gnorm"): 1.08, (100, 33, "fnorm"): 1.53,
                   (256, 63, "prered"): 1.17}


@pytest.mark.parametrize("m,n,kind", [(m, n, "random") for m, n in L.STEP_SHAPES] + [(m, n, "rank1") for m, n in L.STEP_SHAPES if n > 1])
def test_one_step_is_the_trust_region_search_and_the_restatement(qr, plan, m, n, kind):
    b = 5
    J, f, x = _step_case(m, n, b, kind)
    opt = dict(par_rtol=0.1, par_maxit=10)
    lm = qr.LmBatched(plan, m, n, b, **opt)
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        dJ, dF, dX = _dev(J.transpose(0, 2, 1)), _dev(f), _dev(x)
        jp = torch.zeros((b, n), dtype=torch.int32, device="cuda")
        tau = torch.zeros((b, n), dtype=torch.float64, device="cuda")
        lm.start(dX)
        st = lm.state()
        later = [q for q in range(b) if q % 2 == 1]
        for q in later:
            _plant_later(st, q)
        before = _host(st)
        plan.geqp3_batched(dJ, m, n, m, m * n, jp, n, tau, n, b)
        plan.ormqr_batched("T", dJ, m, n, m, m * n, tau, n, dF, 1, m, m, b)
        plan.lm_step_batched(lm, dJ, m, m * n, dF, m, m, m, djpvt=jp, stridejpvt=n)
        plan.sync()
        got = _host(st)
        # the search of section 8g on the same factors: D as the step left it, the radius the search ran on, the start as a lambda
        delta = np.where(before["njev"] == 0, np.where(got["xnorm"] == 0, 100.0, 100.0 * got["xnorm"]), before["delta"])
        X = torch.zeros((b, n), dtype=torch.float64, device="cuda")
        lam, xn = (torch.zeros(b, dtype=torch.float64, device="cuda") for _ in range(2))
        stt, info = (torch.zeros(b, dtype=torch.int32, device="cuda") for _ in range(2))
        plan.trust_batched(dJ, n, m, m * n, dF, m, m, _dev(delta), 1, X, n, n, lam, info, b, djpvt=jp, stridejpvt=n, dD=st["D"], strideD=n,
                           dlam0=_dev(np.sqrt(before["par"])), stridelam0=1, rtol=0.1, maxit=10, dxnorm=xn, dstatus=stt)
        plan.sync()
        P, lam, xn, stt, info = X.cpu().numpy(), lam.cpu().numpy(), xn.cpu().numpy(), stt.cpu().numpy(), info.cpu().numpy()
    lm.close()
    assert not info.any() and not got["info"].any() and not got["status"].any()
    assert np.array_equal(got["xtrial"], before["x"] - P), "xtrial = x - p, p bitwise the search's"
    assert np.array_equal(np.sqrt(got["par"]), lam) and np.array_equal(got["pnorm"], xn) and np.array_equal(got["par_status"], stt)
    assert np.array_equal(got["delta"], np.where(before["iter"] == 1, np.minimum(delta, xn), delta))
    assert np.array_equal(got["njev"], before["njev"] + 1) and np.array_equal(got["x"], before["x"])
    for k in ("iter", "nfev", "accepted"):
        assert np.array_equal(got[k], before[k])
    if kind == "rank1":
        return                                # (the step of a rank-1 J is the rounding of its factorisation: nothing to compare it with)
    worst = {}
    for q in range(b):
        ref = {}
        for dt in (np.float64, L.LD):
            mem = L.Member(x[q], dt, **opt)
            if q in later:
                mem.iter, mem.njev, mem.nfev = 3, 2, 3
                mem.delta, mem.par, mem.xnorm = mem.c(0.375), mem.c(0.0625), mem.c(1.0)
                mem.D = H.arr(np.full(n, 0.5), dt)
            mem.step(J[q], f[q])
            ref[dt] = mem
        r64, rld = ref[np.float64], ref[L.LD]
        assert (r64.par_status, r64.status, r64.info) == (rld.par_status, rld.status, rld.info) == (got["par_status"][q], 0, 0)
        for k in ("xtrial", "D", "delta", "gnorm", "prered", "dirder", "fnorm", "pnorm"):
            e, e64 = _rel(got[k][q], getattr(rld, k)), _rel(np.asarray(getattr(r64, k), dtype=np.float64), getattr(rld, k))
            worst[k] = max(worst.get(k, (0.0, 0.0)), (e / ((m + n) * EPS), e / max(4 * e64, EPS / 4)))
    print(f"\nstep {m}x{n}: worst error / ((m + n) eps), worst error / max(4 x float64's, eps / 4): "
          + ", ".join(f"{k} {v[0]:.2f} {v[1]:.2f}" for k, v in worst.items()))
    for k, (cap, ratio) in worst.items():
        assert cap <= 1.0, (k, cap)
        assert ratio <= max(1.0, STEP_EXCEPTIONS.get((m, n, k), 0.0)), (k, ratio)


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. one update, exactly
# ----------------------------------------------------------------------------------------------------------------------------------
# name -> planted (fnorm, fnorm1, prered, dirder, par, delta, pnorm, gnorm, nfev) and what must come out (accepted, status); x = (3, 4, 0),
# xtrial = (6, 8, 0), D = 1: the norms are exact
T_A = dict(  # options: the defaults, maxfev 7
    low_ratio_actred_pos=((1.0, 0.99, 0.5, -0.4, 0.25, 2.0, 1.5, 0.5, 2), (1, 0)),
    low_ratio_actred_neg=((1.0, 1.05, 0.5, -0.4, 0.25, 2.0, 1.5, 0.5, 2), (0, 0)),
    floor_by_temp=((1.0, 3.0, 0.5, -0.4, 0.25, 2.0, 1.5, 0.5, 2), (0, 0)),
    floor_by_tenfold=((1.0, 20.0, 0.5, -0.4, 0.25, 2.0, 1.5, 0.5, 2), (0, 0)),
    high_ratio=((1.0, 0.5, 0.8, -0.6, 0.25, 2.0, 1.5, 0.5, 2), (1, 0)),
    par_zero=((1.0, 0.8, 0.8, -0.6, 0.0, 2.0, 1.5, 0.5, 2), (1, 0)),
    mid_ratio_no_change=((1.0, 0.8, 0.8, -0.6, 0.25, 2.0, 1.5, 0.5, 2), (1, 0)),
    prered_zero=((1.0, 0.8, 0.0, 0.0, 0.25, 2.0, 1.5, 0.5, 2), (0, 0)),
    ftrial_nan=((1.0, float("nan"), 0.5, -0.4, 0.25, 2.0, 1.5, 0.5, 2), (0, 0)),
    ftrial_inf=((1.0, float("inf"), 0.5, -0.4, 0.25, 2.0, 1.5, 0.5, 2), (0, 0)),
    stop_1=((1.0, 1.0 - 1e-10, 3e-10, -2e-10, 0.25, 2.0, 1.5, 0.5, 2), (1, 1)),
    stop_2=((1.0, 0.8, 0.8, -0.6, 0.25, 1e-9, 1e-9, 0.5, 2), (1, 2)),
    stop_3=((1.0, 1.0 - 1e-10, 3e-10, -2e-10, 0.25, 1e-9, 1e-9, 0.5, 2), (1, 3)),
    stop_5=((1.0, 0.8, 0.8, -0.6, 0.25, 2.0, 1.5, 0.5, 6), (1, 5)),
)
T_B = dict(  # options: ftol = xtol = 0
    stop_6=((1.0, 1.0, 1e-17, -1e-17, 0.25, 2.0, 1.5, 0.5, 2), (0, 6)),
    stop_7=((1.0, 0.8, 0.8, -0.6, 0.25, 1e-16, 1e-16, 0.5, 2), (1, 7)),
    stop_8=((1.0, 0.8, 0.8, -0.6, 0.25, 2.0, 1.5, 1e-17, 2), (1, 8)),
    none=((1.0, 0.8, 0.8, -0.6, 0.25, 2.0, 1.5, 0.5, 2), (1, 0)),
)
PLANTED = ("fnorm", "fnorm1", "prered", "dirder", "par", "delta", "pnorm", "gnorm", "nfev")


@pytest.mark.parametrize("table,opt", [(T_A, dict(maxfev=7)), (T_B, dict(ftol=0.0, xtol=0.0))], ids=["defaults", "zero_tolerances"])
def test_one_update_is_bitwise_the_restatement_on_every_branch(qr, plan, table, opt):
    names = list(table)
    b, m, n = len(names), 4, 3
    lm = qr.LmBatched(plan, m, n, b, **opt)
    x, xt = np.array([3.0, 4.0, 0.0]), np.array([6.0, 8.0, 0.0])
    Ft = np.zeros((b, m))
    refs = []
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        lm.start(_dev(np.tile(x, (b, 1))))
        st = lm.state()
        J = _dev(np.tile(np.eye(m, n).T, (b, 1, 1)))
        lm.step(J, _dev(np.ones((b, m))))     # (any step: the phase flag lives on the host; the state it leaves is replaced below)
        for q, name in enumerate(names):
            v = dict(zip(PLANTED, table[name][0]))
            mem = L.Member(x, np.float64, **opt)
            mem.xtrial, mem.njev, mem.iter, mem.nfev = xt.copy(), 2, 2, v["nfev"]
            mem.xnorm = 5.0
            for k in ("fnorm", "prered", "dirder", "par", "delta", "pnorm", "gnorm"):
                setattr(mem, k, np.float64(v[k]))
            for k in L.SCALARS + L.COUNTERS:
                st[k][q] = float(getattr(mem, k)) if k in L.SCALARS else int(getattr(mem, k))
            st["x"][q], st["xtrial"][q], st["D"][q] = _dev(x), _dev(xt), 1.0
            Ft[q, 0] = v["fnorm1"]
            mem.D = np.ones(n)
            mem.update(Ft[q])
            refs.append(mem)
        lm.update(_dev(Ft))
        plan.sync()
        got = _host(st)
    lm.close()
    for q, name in enumerate(names):
        mem = refs[q]
        assert (mem.accepted, mem.status) == table[name][1], (name, mem.accepted, mem.status)         # the tuple reaches its branch
        for k in L.SCALARS + L.COUNTERS:
            assert np.array_equal(got[k][q], np.asarray(getattr(mem, k)).astype(got[k].dtype), equal_nan=True), (name, k, got[k][q], getattr(mem, k))
        assert np.array_equal(got["x"][q], mem.x) and np.array_equal(got["xtrial"][q], xt), name


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. whole solves
# ----------------------------------------------------------------------------------------------------------------------------------
# problem -> the worst ratio of |x - x_longdouble| to 4 x the float64 restatement's, where it exceeds 1 (measured on an MI355X)
# (powell: 2.6e-10 of the condition bound; kappa reaches 1e8 on the way to the singular solution)
SOLVE_EXCEPTIONS = {"powell": 4.22}


@pytest.mark.parametrize("name", sorted(L.PROBLEMS))
def test_whole_solves_take_the_restatements_decisions(qr, plan, name):
    p = L.PROBLEMS[name]
    x0, data, xs, r64, rld = _ref(name)
    got = _solve(qr, plan, p, x0, data, **p.options)
    worst, worst4 = 0.0, 0.0
    for q in range(p.batch):
        a, l = r64[q], rld[q]
        assert (got["status"][q], got["nfev"][q], got["njev"][q], got["iter"][q], got["info"][q]) == (a.status, a.nfev, a.njev, a.iter, 0), q
        e, e64 = _rel(got["x"][q], l.x), _rel(np.asarray(a.x, dtype=np.float64), l.x)
        cap = 50 * a.kappa * EPS * a.iter
        worst, worst4 = max(worst, e / cap if cap else (0.0 if e == 0 else np.inf)), max(worst4, e / max(4 * e64, EPS / 4))
        if p.planted:
            assert np.linalg.norm(got["x"][q] - xs[q]) <= 100 * L.DEFAULTS["xtol"] * np.linalg.norm(xs[q]), q
    print(f"\nsolve {name}: batch {p.batch}, status {sorted(set(got['status']))}, nfev {got['nfev'].min()}..{got['nfev'].max()}, "
          f"worst |x - x_ld| / (50 kappa eps iter |x|) {worst:.2e}, / max(4 x float64's, eps / 4) {worst4:.2f}")
    assert worst <= 1.0
    assert worst4 <= max(1.0, SOLVE_EXCEPTIONS.get(name, 0.0))


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. mixed batch
# ----------------------------------------------------------------------------------------------------------------------------------
class Mixed(L.Problem):
    """members of three problems of one shape in one batch: kind[q] picks the model of member q (the data carries it in column m)"""
    m, n = 16, 3

    def __init__(self):
        self.parts = [L.ExpDecay(16), L.LinearFullRank(16, 3), L.LinearRank1(16, 3)]

    def f(self, xp, x, data):
        kind = data[..., self.m:self.m + 1]
        out = 0
        for i, p in enumerate(self.parts):
            out = out + (kind == i) * p.f(xp, x, data[..., :self.m])
        return out

    def jac(self, xp, x, data):
        kind = data[..., self.m:self.m + 1, None]
        out = 0
        for i, p in enumerate(self.parts):
            out = out + (kind == i) * p.jac(xp, x, data[..., :self.m])
        return out

    def members(self, count):
        x0, data = [], []
        for q in range(count):
            i = q % 3
            a, d, _ = self.parts[i].members(q + 1)
            x0.append(a[q])
            data.append(np.concatenate([np.zeros(16) if d is None else d[q], [float(i)]]))
        return np.stack(x0), np.stack(data), None


def test_mixed_batch_frozen_members_and_independence_of_batch_and_index(qr, plan):
    p = Mixed()
    x0, data, _ = p.members(9)
    opt = dict(gtol=1e-8)
    full, tr = _solve(qr, plan, p, x0, data, trace=True, **opt)
    assert not full["info"].any() and (full["status"] > 0).all()
    assert len(set(full["nfev"])) >= 3, "the members run different numbers of rounds"
    print(f"\nmixed: status {full['status']}, nfev {full['nfev']}")
    for q in range(9):                        # from the round a member finished in, its whole state is frozen
        done = next(i for i, s in enumerate(tr) if s["status"][q] != 0)
        for s in tr[done + 1:]:
            assert _same(s, tr[done], q=q, r=q) is None, (q, _same(s, tr[done], q=q, r=q))
    again = _solve(qr, plan, p, x0, data, **opt)
    assert _same(again, full) is None, "repeats are bitwise equal"
    for idx in ([8, 3, 0, 5, 2], [4], [6, 7, 1]):
        part = _solve(qr, plan, p, x0[idx], data[idx], **opt)
        for r, q in enumerate(idx):
            assert _same(full, part, q=q, r=r) is None, (idx, q, _same(full, part, q=q, r=r))


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. a trial point that is NaN or inf; a scaling of mode 2 that is not positive
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,who,when", [(float("nan"), 2, 1), (float("inf"), 3, 0)])
def test_a_member_whose_trial_point_is_not_finite(qr, plan, bad, who, when):
    p = L.PROBLEMS["expdecay16"]
    x0, data, xs = p.members(5)

    def hook(rounds, Ft):
        if rounds == when:
            Ft = Ft.clone()
            Ft[who] = bad
        return Ft

    clean = _solve(qr, plan, p, x0, data)
    got, tr = _solve(qr, plan, p, x0, data, trace=True, hook=hook)
    step, upd = tr[2 * when], tr[2 * when + 1]
    assert upd["accepted"][who] == 0 and upd["status"][who] == 0 and upd["iter"][who] == step["iter"][who]
    assert np.array_equal(upd["x"][who], step["x"][who])
    assert upd["delta"][who] == 0.1 * min(step["delta"][who], step["pnorm"][who] / 0.1) < step["delta"][who]
    assert upd["par"][who] == step["par"][who] / 0.1
    assert got["status"][who] in (1, 2, 3, 4, 5) and got["info"][who] == 0
    if got["status"][who] != 5:               # it recovers: the planted x
        assert np.linalg.norm(got["x"][who] - xs[who]) <= 100 * L.DEFAULTS["xtol"] * np.linalg.norm(xs[who])
    print(f"\nnon-finite trial point ({bad}): status {got['status'][who]}, nfev {got['nfev'][who]} (clean: {clean['nfev'][who]})")
    for q in range(5):
        if q != who:
            assert _same(got, clean, q=q, r=q) is None, (q, _same(got, clean, q=q, r=q))


def test_a_scaling_of_mode_2_that_is_not_positive(qr, plan):
    p = L.PROBLEMS["expdecay16"]
    x0, data, xs = p.members(5)
    D = np.ones((5, 3))
    clean = _solve(qr, plan, p, x0, data, D0=D, mode=2)
    D[1, 1], D[3, 2] = 0.0, -1.0
    got = _solve(qr, plan, p, x0, data, D0=D, mode=2)
    for q in (1, 3):
        assert got["info"][q] == -1 and got["status"][q] == 0
        assert np.array_equal(got["x"][q], x0[q]) and np.array_equal(got["xtrial"][q], x0[q]) and np.array_equal(got["D"][q], D[q])
        assert (got["iter"][q], got["nfev"][q], got["njev"][q], got["accepted"][q], got["par_status"][q]) == (1, 1, 0, 0, 0)
        assert all(got[k][q] == 0 for k in L.SCALARS)
    for q in (0, 2, 4):
        assert got["status"][q] > 0 and _same(got, clean, q=q, r=q) is None, q


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. scale equivariance
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["expdecay16", "rosenbrock", "linfull64x32"])
@pytest.mark.parametrize("e", [20, -20])
def test_scaling_f_and_J_by_a_power_of_two(qr, plan, name, e):
    p = L.PROBLEMS[name]
    x0, data, _ = p.members(p.batch)
    s = 2.0 ** e
    one, tr1 = _solve(qr, plan, p, x0, data, trace=True, **p.options)
    two, tr2 = _solve(qr, plan, p, x0, data, trace=True, scale=s, **p.options)
    assert len(tr1) == len(tr2)
    for a, c in zip(tr1, tr2):
        assert _same(a, c, keys=("x", "xtrial", "par", "gnorm", "prered", "dirder") + L.COUNTERS) is None
        for k in ("fnorm", "delta", "pnorm", "xnorm", "D"):
            assert np.array_equal(a[k] * s, c[k]), k
    assert (one["status"] > 0).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 7. from factors and from an accumulator
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(16, 3), (64, 31), (100, 33)])
def test_step_from_factors_is_the_third_launch_of_the_step(qr, plan, m, n):
    b = 5
    J, f, x = _step_case(m, n, b, "random")
    outs = []
    for way in ("step", "factors"):
        lm = qr.LmBatched(plan, m, n, b)
        with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
            dJ, dF = _dev(J.transpose(0, 2, 1)), _dev(f)
            lm.start(_dev(x))
            if way == "step":
                lm.step(dJ, dF)
            else:
                jp = torch.zeros((b, n), dtype=torch.int32, device="cuda")
                tau = torch.zeros((b, n), dtype=torch.float64, device="cuda")
                plan.geqp3_batched(dJ, m, n, m, m * n, jp, n, tau, n, b)
                plan.ormqr_batched("T", dJ, m, n, m, m * n, tau, n, dF, 1, m, m, b)
                plan.lm_step_batched(lm, dJ, m, m * n, dF, m, m, m, djpvt=jp, stridejpvt=n)
            plan.sync()
            outs.append((_host(lm.state()), dJ.cpu().numpy(), dF.cpu().numpy()))
        lm.close()
    assert _same(outs[0][0], outs[1][0]) is None
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2]), "dJ as geqp3 leaves it, dF as Q^T f"
    assert (outs[0][0]["njev"] == 1).all() and not outs[0][0]["info"].any()


@pytest.mark.parametrize("m,n", [(16, 3), (100, 33)])
def test_step_from_an_accumulators_factors(qr, plan, m, n):
    b = 5
    J, f, x = _step_case(m, n, b, "random")
    acc = qr.LsAccumulatorBatched(plan, n, 1, b)
    outs = []
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        acc.push(_dev(J.transpose(0, 2, 1)), m, m, m * n, _dev(f), m, m)
        r, ldr, sr, z, ldz, sz, rss, _ = acc.factor()
        R, Z, S, _rows = acc.factor_host()
        for way in ("state", "copies"):
            lm = qr.LmBatched(plan, m, n, b)
            lm.start(_dev(x))
            if way == "state":
                plan.lm_step_batched(lm, r, ldr, sr, z, n, ldz, sz, drss=rss)
            else:                             # the same numbers at another leading dimension and stride
                ld = n + 3
                Rp = np.full((b, n, ld), -7.25e33)
                Rp[:, :, :n] = R.transpose(0, 2, 1)
                Zp = np.full((b, ld), -7.25e33)
                Zp[:, :n] = Z[:, :, 0]
                keep = (_dev(Rp), _dev(Zp), _dev(S[:, 0]))
                plan.lm_step_batched(lm, keep[0], ld, n * ld, keep[1], n, ld, ld, drss=keep[2])
            plan.sync()
            outs.append(_host(lm.state()))
            lm.close()
    acc.close()
    assert _same(outs[0], outs[1]) is None
    got = outs[0]
    assert not got["info"].any() and (got["njev"] == 1).all()
    for q in range(b):
        mem = L.Member(x[q], L.LD)
        mem.step_factors(R[q], Z[q, :, 0], None, S[q, 0])
        for k in ("xtrial", "D", "delta", "gnorm", "prered", "dirder", "fnorm"):
            assert _rel(got[k][q], getattr(mem, k)) <= (m + n) * EPS, (q, k, _rel(got[k][q], getattr(mem, k)) / EPS)


# ----------------------------------------------------------------------------------------------------------------------------------
# 8. the host twin and lm_batched
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["expdecay16", "rosenbrock", "linfull64x32", "powell"])
def test_host_twin_and_torch_driver_return_what_the_handle_returns(qr, plan, name):
    p = L.PROBLEMS[name]
    x0, data, xs, r64, rld = _ref(name)
    base = _solve(qr, plan, p, x0, data, **p.options)
    dat = _dev(data)
    out = qr.lm_batched(lambda x: p.f(torch, x, dat), lambda x: p.jac(torch, x, dat), _dev(x0), check_every=3, **p.options)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got["status"] > 0).all()
    assert _same(got, base, keys=("x", "fnorm", "status", "nfev", "njev", "iter", "info")) is None, "the same kernels on the same model"
    X, fnorm, nfev, njev, status, info = qr.lstsq_lm_batched(lambda x: p.f(np, x, data), lambda x: p.jac(np, x, data), x0, m=p.m, **p.options)
    assert np.array_equal(status, base["status"]) and np.array_equal(nfev, base["nfev"]) and np.array_equal(njev, base["njev"])
    assert not info.any()
    for q in range(p.batch):                  # (the model runs in numpy here and in torch there: equal to the rounding of the model)
        assert _rel(X[q], rld[q].x) <= 50 * r64[q].kappa * EPS * r64[q].iter, q
    assert np.isfinite(fnorm).all()
