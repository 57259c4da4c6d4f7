"""-m gpu: the bounded batched Levenberg-Marquardt solver (mi355x_qr.h section 8n), member by member.

Problems, their starts, bounds and options, and the restatement: tests/batched_lmb_ref.py; tests/test_batched_lmb_ref.py shows on the CPU
that the float64 and the longdouble restatement take the same decisions on every member used here, that no peg decision sits within 64 m
eps |J_j| |f| of a sign change, and that the members end at the KKT points scipy finds -- the conditions under which the solves below
demand equal counts, pegs and clipped words.

What ties the solver to section 8m: with every bound infinite every state array is bitwise LmBatched's after every call.

Figures are printed (-s) before they are asserted; DESIGN.md section 7w tabulates them."""
import functools

import numpy as np
import pytest
import torch

import batched_lm_ref as L
import batched_lmb_ref as B
import hp_ref as H

pytestmark = pytest.mark.gpu

EPS = L.EPS
DOUBLES = ("x", "xtrial", "D") + L.SCALARS
STATE = DOUBLES + L.COUNTERS
BSTATE = STATE + B.EXTRA
MAX_ROUNDS = 700
UNIT = ("gnorm", "prered", "dirder", "alpha")     # cosines, relative reductions and a fraction: their errors are measured against 1


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


def _host(st, keys):
    return {k: st[k].cpu().numpy().copy() for k in keys}


def _same(a, b, keys, q=None, r=None):
    """bitwise equality of two states (member q of a against member r of b): None, or the first key that differs"""
    for k in keys:
        x, y = (a[k] if q is None else a[k][q]), (b[k] if r is None else b[k][r])
        if not np.array_equal(x, y, equal_nan=True):
            return k
    return None


def _solve(qr, plan, prob, x0, data, lo=None, hi=None, bounded=True, trace=False, scale=1.0, watch=None, **options):
    """every member through LmBoundedBatched (or LmBatched) with the model in torch on the plan's stream: the final state, and with trace
    the state after every step and after every update.  watch(lm, st, Jbefore, J): called after every step"""
    b, n = x0.shape
    m = prob.m
    lm = (qr.LmBoundedBatched if bounded else qr.LmBatched)(plan, m, n, b, **options)
    keys = BSTATE if bounded else STATE
    tr = []
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        X0, dat = _dev(x0), _dev(data)
        if bounded:
            lm.start(X0, dLo=_dev(lo), dHi=_dev(hi))
        else:
            lm.start(X0)
        st = lm.state()
        J = torch.empty((b, n, m), dtype=torch.float64, device="cuda")
        F = torch.empty((b, m), dtype=torch.float64, device="cuda")
        rounds = 0
        while True:
            J.copy_((scale * prob.jac(torch, st["x"], dat)).transpose(1, 2))
            F.copy_(scale * prob.f(torch, st["x"], dat))
            Jb = J.clone() if watch else None
            lm.step(J, F)
            if watch:
                watch(lm, st, Jb, J)
            if trace:
                tr.append(_host(st, keys))
            F.copy_(scale * prob.f(torch, st["xtrial"], dat))
            lm.update(F)
            if trace:
                tr.append(_host(st, keys))
            rounds += 1
            if lm.running() == 0 or rounds >= MAX_ROUNDS:
                break
        out = _host(st, keys)
    lm.close()
    assert rounds < MAX_ROUNDS
    return (out, tr) if trace else out


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the members of a problem at its batch size (x0, data, lo, hi) with their float64 and longdouble restatements, once"""
    p = B.PROBLEMS[name]
    return B.good_members(p, p.batch)


def _err(got, ref, key):
    a, b = H.arr(got), H.arr(ref)
    d, s = float(H.norm(a - b)), float(H.norm(b))
    if key in UNIT:
        s = max(s, 1.0)
    return d / s if s else d


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. every bound infinite: section 8m, bitwise, after every call
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f"linbox{m}x{n}" for m, n in B.SHAPES] + ["expdecay_b", "gausspeak_b", "rosenbrock_b"])
@pytest.mark.parametrize("how", ["null", "inf"])
def test_with_every_bound_infinite_every_state_array_is_lm_batcheds_after_every_call(qr, plan, name, how):
    p = B.PROBLEMS[name]
    x0, data, lo, hi, _r64, _rld = _ref(name)
    want, trw = _solve(qr, plan, p, x0, data, bounded=False, trace=True, **p.options)
    free = (None, None) if how == "null" else (np.full_like(x0, -np.inf), np.full_like(x0, np.inf))
    got, trg = _solve(qr, plan, p, x0, data, free[0], free[1], trace=True, **p.options)
    assert len(trw) == len(trg)
    for i, (a, c) in enumerate(zip(trg, trw)):
        assert _same(a, c, STATE) is None, (i, _same(a, c, STATE))
        assert not a["peg"].any() and not a["clipped"].any() and (a["alpha"] == 1.0).all()
    assert (want["status"] > 0).all() and _same(got, want, STATE) is None


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. bounded solves
# ----------------------------------------------------------------------------------------------------------------------------------
# (problem, quantity) -> the worst ratio of the error against the longdouble restatement to 4 x the float64 restatement's, where it
# exceeds 1 (measured on an MI355X; where the float64 restatement happens to land within eps / 16 of the longdouble one the yardstick is
# eps / 4, and the largest figure, 10.36, is then an error of 2.6 eps)
SOLVE_EXCEPTIONS = {("expdecay_b", "delta"): 1.87, ("expdecay_b", "xnorm"): 3.22, ("expdecay_b", "pnorm"): 1.87, ("gausspeak_b", "x"): 1.35,
                    ("gausspeak_b", "delta"): 4.2, ("gausspeak_b", "fnorm"): 5.07, ("gausspeak_b", "xnorm"): 3.65, ("gausspeak_b", "pnorm"): 4.2,
                    ("linbox100x33", "delta"): 4.54, ("linbox100x33", "xnorm"): 2.34, ("linbox100x33", "pnorm"): 4.54, ("linbox16x3", "delta"): 2.92,
                    ("linbox16x3", "pnorm"): 2.92, ("linbox16x7", "fnorm"): 4.56, ("linbox16x7", "gnorm"): 1.35, ("linbox16x7", "prered"): 5.22,
                    ("linbox16x7", "dirder"): 5.22, ("linbox24x6", "delta"): 5.67, ("linbox24x6", "pnorm"): 5.67, ("linbox24x6", "prered"): 6.48,
                    ("linbox24x6", "dirder"): 6.48, ("linbox24x8", "delta"): 6.1, ("linbox24x8", "fnorm"): 1.09, ("linbox24x8", "xnorm"): 2.18,
                    ("linbox24x8", "pnorm"): 6.1, ("linbox3x1", "delta"): 10.37, ("linbox3x1", "pnorm"): 10.37, ("linbox3x1", "prered"): 2.26,
                    ("linbox3x1", "dirder"): 9.86, ("linbox3x1", "alpha"): 5.08, ("linbox64x31", "fnorm"): 1.78, ("linbox65x16", "delta"): 1.04,
                    ("linbox65x16", "pnorm"): 1.04}


@pytest.mark.parametrize("name", sorted(B.PROBLEMS))
def test_bounded_solves_take_the_restatements_decisions(qr, plan, name):
    p = B.PROBLEMS[name]
    x0, data, lo, hi, r64, rld = _ref(name)
    got, tr = _solve(qr, plan, p, x0, data, lo, hi, trace=True, **p.options)
    worst = {}
    for q in range(p.batch):
        a, l = r64[q], rld[q]
        assert (got["status"][q], got["nfev"][q], got["njev"][q], got["iter"][q], got["info"][q]) == (a.status, a.nfev, a.njev, a.iter, 0), q
        assert np.array_equal(got["peg"][q], a.peg) and (got["clipped"][q], got["accepted"][q]) == (a.clipped, a.accepted), q
        x = got["x"][q]
        assert np.all(x >= lo[q]) and np.all(x <= hi[q]), q
        assert np.array_equal(x[a.peg == -1], lo[q][a.peg == -1]) and np.array_equal(x[a.peg == 1], hi[q][a.peg == 1]), q
        for k in ("x",) + L.SCALARS + ("alpha",):
            e, e64 = _err(got[k][q], getattr(l, k), k), _err(np.asarray(getattr(a, k), dtype=np.float64), getattr(l, k), k)
            worst[k] = max(worst.get(k, 0.0), e / max(4 * e64, EPS / 4))
    fixed = lo == hi
    for s in tr:                              # a fixed parameter never moves, and no point ever leaves the box
        assert np.array_equal(s["x"][fixed], lo[fixed]) and np.array_equal(s["xtrial"][fixed], lo[fixed])
        run = s["info"] == 0
        assert np.all(s["xtrial"][run] >= lo[run]) and np.all(s["xtrial"][run] <= hi[run])
    print(f"\nbounded solve {name}: batch {p.batch}, status {sorted(set(got['status']))}, nfev {got['nfev'].min()}..{got['nfev'].max()}, "
          f"held {[int((got['peg'][q] != 0).sum()) for q in range(p.batch)]}; worst error / max(4 x float64's, eps / 4): "
          + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= max(1.0, SOLVE_EXCEPTIONS.get((name, k), 0.0)), (k, v)


@pytest.mark.parametrize("m,n", B.SHAPES)
def test_linear_box_members_agree_with_bvls_on_the_device(qr, plan, m, n):
    name = f"linbox{m}x{n}"
    p = B.PROBLEMS[name]
    x0, data, lo, hi, r64, rld = _ref(name)
    b = p.batch
    assert m <= qr.bvls_batched_max_rows(n)
    got = _solve(qr, plan, p, x0, data, lo, hi, **p.options)
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        dA, dB = _dev(data[:, :m * n]), _dev(data[:, m * n:])
        X = torch.zeros((b, n), dtype=torch.float64, device="cuda")
        info = torch.zeros(b, dtype=torch.int32, device="cuda")
        plan.bvls_batched(dA, m, n, m, m * n, dB, m, X, n, info, b, dlo=_dev(lo), dhi=_dev(hi), stridebnd=n)
        plan.sync()
        xb, info = X.cpu().numpy(), info.cpu().numpy()
    assert not info.any()
    worst = max(np.linalg.norm(got["x"][q] - xb[q]) / np.linalg.norm(xb[q]) for q in range(b))
    print(f"\n{name}: worst |x - x_bvls| / |x_bvls| {worst:.2e} (cap {B.BVLS_CAP:.2e})")
    assert worst <= B.BVLS_CAP


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. bad inputs: info -2, nothing else written, the neighbours unaffected
# ----------------------------------------------------------------------------------------------------------------------------------
def _bad_start(qr, plan, spoil):
    """expdecay_b, five members: a clean solve, then a solver that is started clean, stepped once, and restarted with member 2 spoiled"""
    p = B.PROBLEMS["expdecay_b"]
    x0, data, lo, hi, _r64, _rld = _ref("expdecay_b")
    x0, data, lo, hi = x0[:5].copy(), data[:5], lo[:5].copy(), hi[:5].copy()
    clean = _solve(qr, plan, p, x0, data, lo, hi, **p.options)
    b, n, m = 5, p.n, p.m
    lm = qr.LmBoundedBatched(plan, m, n, b, **p.options)
    with torch.cuda.stream(torch.cuda.ExternalStream(plan.stream)):
        dat = _dev(data)
        lm.start(_dev(x0), dLo=_dev(lo), dHi=_dev(hi))
        st = lm.state()
        J = torch.empty((b, n, m), dtype=torch.float64, device="cuda")
        F = torch.empty((b, m), dtype=torch.float64, device="cuda")

        def round_():
            J.copy_(p.jac(torch, st["x"], dat).transpose(1, 2))
            F.copy_(p.f(torch, st["x"], dat))
            lm.step(J, F)
            F.copy_(p.f(torch, st["xtrial"], dat))
            lm.update(F)

        round_()
        lm.running()
        before = _host(st, BSTATE)
        spoil(x0, lo, hi)
        lm.start(_dev(x0), dLo=_dev(lo), dHi=_dev(hi))
        lm.running()
        after = _host(st, BSTATE)
        rounds = 0
        while lm.running() and rounds < MAX_ROUNDS:
            round_()
            rounds += 1
        end = _host(st, BSTATE)
    lm.close()
    assert after["info"][2] == -2 and end["info"][2] == -2
    keys = tuple(k for k in BSTATE if k != "info")
    assert _same(after, before, keys, q=2, r=2) is None, _same(after, before, keys, q=2, r=2)      # nothing else is written
    assert _same(end, before, keys, q=2, r=2) is None, "skipped from then on"
    for q in (0, 1, 3, 4):
        assert end["status"][q] > 0 and _same(end, clean, BSTATE, q=q, r=q) is None, (q, _same(end, clean, BSTATE, q=q, r=q))


def test_info_minus_2_for_a_lower_bound_above_the_upper(qr, plan):
    def spoil(x0, lo, hi):
        lo[2, 0], hi[2, 0] = 3.0, 2.0
    _bad_start(qr, plan, spoil)


def test_info_minus_2_for_a_nan_bound(qr, plan):
    def spoil(x0, lo, hi):
        hi[2, 2] = np.nan
    _bad_start(qr, plan, spoil)


def test_info_minus_2_for_a_start_outside_the_box(qr, plan):
    def spoil(x0, lo, hi):
        x0[2, 1] = hi[2, 1] * (1.0 + 2.0 ** -40)
    _bad_start(qr, plan, spoil)


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. finished members; repeats, the batch size and the index; scaling
# ----------------------------------------------------------------------------------------------------------------------------------
def test_a_finished_members_state_and_columns_of_J_are_left_untouched_by_the_peg(qr, plan):
    """the factorisation still runs on the slots of a finished member, so its J is compared with the factors of the J that went in: equal
    bit for bit for a finished member (no column was cleared), different for a running member with a held column"""
    name = "linbox16x7"
    p = B.PROBLEMS[name]
    x0, data, lo, hi, r64, _rld = _ref(name)
    b, m, n = p.batch, p.m, p.n
    seen = dict(finished=0, held=0)
    jp = torch.zeros((b, n), dtype=torch.int32, device="cuda")
    tau = torch.zeros((b, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def watch(lm, st, Jb, J):
        plan.geqp3_batched(Jb, m, n, m, m * n, jp, n, tau, n, b)
        plan.sync()
        same = (Jb == J).flatten(1).all(1).cpu().numpy()
        status, peg = st["status"].cpu().numpy(), st["peg"].cpu().numpy()
        for q in range(b):
            done_before = status[q] != 0 and watch.prev is not None and watch.prev["status"][q] != 0
            if done_before:
                assert same[q], q
                seen["finished"] += 1
            elif peg[q].any():
                assert not same[q], q
                seen["held"] += 1
        watch.prev = _host(st, BSTATE)

    watch.prev = None
    full, tr = _solve(qr, plan, p, x0, data, lo, hi, trace=True, watch=watch, **p.options)
    assert seen["finished"] > 0 and seen["held"] > 0, seen
    assert len(set(full["nfev"])) >= 2, "the members run different numbers of rounds"
    for q in range(b):                        # from the round a member finished in, its whole state is frozen
        done = next(i for i, s in enumerate(tr) if s["status"][q] != 0)
        for s in tr[done + 1:]:
            assert _same(s, tr[done], BSTATE, q=q, r=q) is None, (q, _same(s, tr[done], BSTATE, q=q, r=q))


@pytest.mark.parametrize("name", ["linbox24x8", "gausspeak_b", "linbox100x33"])
def test_results_are_repeatable_and_independent_of_the_batch_size_and_the_index(qr, plan, name):
    p = B.PROBLEMS[name]
    x0, data, lo, hi, _r64, _rld = _ref(name)
    full = _solve(qr, plan, p, x0, data, lo, hi, **p.options)
    again = _solve(qr, plan, p, x0, data, lo, hi, **p.options)
    assert _same(again, full, BSTATE) is None, "repeats are bitwise equal"
    b = p.batch
    for idx in ([b - 1, 3, 0, 2], [4], [1, 2]):
        part = _solve(qr, plan, p, x0[idx], data[idx], lo[idx], hi[idx], **p.options)
        for r, q in enumerate(idx):
            assert _same(full, part, BSTATE, q=q, r=r) is None, (idx, q, _same(full, part, BSTATE, q=q, r=r))


@pytest.mark.parametrize("name", ["expdecay_b", "rosenbrock_b", "linboxfree100x33"])
@pytest.mark.parametrize("e", [20, -20])
def test_scaling_f_and_J_by_a_power_of_two(qr, plan, name, e):
    """(members without a column held at the first step: such a column gets D_j = 1, MINPACK's rule for a zero column, at every scale)"""
    p = B.PROBLEMS[name]
    x0, data, lo, hi, _r64, _rld = _ref(name)
    s = 2.0 ** e
    one, tr1 = _solve(qr, plan, p, x0, data, lo, hi, trace=True, **p.options)
    two, tr2 = _solve(qr, plan, p, x0, data, lo, hi, trace=True, scale=s, **p.options)
    assert len(tr1) == len(tr2)
    for a, c in zip(tr1, tr2):
        assert _same(a, c, ("x", "xtrial", "par", "gnorm", "prered", "dirder") + L.COUNTERS + B.EXTRA) is None
        for k in ("fnorm", "delta", "pnorm", "xnorm", "D"):
            assert np.array_equal(a[k] * s, c[k]), k
    assert (one["status"] > 0).all()


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. the host twin and lm_batched
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["expdecay_b", "rosenbrock_b", "linbox64x31"])
def test_host_twin_and_torch_driver_return_what_the_handle_returns(qr, plan, name):
    p = B.PROBLEMS[name]
    x0, data, lo, hi, r64, rld = _ref(name)
    base = _solve(qr, plan, p, x0, data, lo, hi, **p.options)
    dat = _dev(data)
    out = qr.lm_batched(lambda x: p.f(torch, x, dat), lambda x: p.jac(torch, x, dat), _dev(x0), check_every=3, bounds=(_dev(lo), _dev(hi)),
                        **p.options)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got["status"] > 0).all()
    keys = ("x", "fnorm", "status", "nfev", "njev", "iter", "info", "peg", "clipped", "alpha", "lo", "hi")
    assert _same(got, base, keys) is None, "the same kernels on the same model"
    X, fnorm, nfev, njev, status, info = qr.lstsq_lm_batched(lambda x: p.f(np, x, data), lambda x: p.jac(np, x, data), x0, m=p.m,
                                                             bounds=(lo, hi), **p.options)
    assert np.array_equal(status, base["status"]) and np.array_equal(nfev, base["nfev"]) and np.array_equal(njev, base["njev"])
    assert not info.any() and np.isfinite(fnorm).all()
    assert np.all(X >= lo) and np.all(X <= hi)
    for q in range(p.batch):                  # (the model runs in numpy here and in torch there: equal to the rounding of the model,
        a = r64[q]                            # carried by the condition of the free columns of J D^-1 at the end)
        d = None if data is None else data[q]
        Jf = (p.jac(np, np.asarray(a.x, dtype=np.float64), d) / np.asarray(a.D, dtype=np.float64))[:, a.peg == 0]
        kappa = np.linalg.cond(Jf) if Jf.shape[1] else 1.0
        assert np.array_equal(X[q][a.peg != 0], base["x"][q][a.peg != 0]), q
        assert _err(X[q], rld[q].x, "x") <= 50 * kappa * EPS * a.iter, (q, _err(X[q], rld[q].x, "x"), kappa)
