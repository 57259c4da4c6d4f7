"""CPU-side checks of the numpy restatement of the bounded batched Levenberg-Marquardt solver (tests/batched_lmb_ref.py; mi355x_qr.h section
8n): with every bound infinite it is batched_lm_ref bit for bit; on the bounded problems it ends at KKT points, the ones
scipy.optimize.least_squares(method="trf") and lsq_linear(method="bvls") find; the float64 and the longdouble instance take the same
decisions, and no peg decision sits within rounding of a sign change -- the conditions under which tests/test_gpu_batched_lmb.py may
demand equal counts and pegs.

Figures are printed (-s) before they are asserted; DESIGN.md section 7w has them."""
import functools

import numpy as np
import pytest

import scipy.optimize as scipy_optimize

import batched_lm_ref as L
import batched_lmb_ref as B

TRF_WORST, TRF_CAP, BVLS_WORST, BVLS_CAP = B.TRF_WORST, B.TRF_CAP, B.BVLS_WORST, B.BVLS_CAP
COUNT = 20


@functools.lru_cache(maxsize=None)
def _runs(name):
    p = B.PROBLEMS[name]
    return (p,) + B.good_members(p, COUNT if name in B.KINDS else p.batch)


def _decisions(mem):
    return (mem.status, mem.nfev, mem.njev, mem.iter, mem.info, tuple(mem.peg), mem.clipped, mem.accepted)


def _free_problem(p, x0, d, lo, hi):
    """the member with its fixed parameters (lo == hi) taken out: fun, jac on the free ones, their bounds and a start strictly inside"""
    free = lo != hi

    def full(xf):
        x = np.array(x0)
        x[free] = xf
        return x

    lof, hif = lo[free], hi[free]
    s = np.clip(x0[free], np.where(np.isfinite(lof), lof + 1e-9, lof), np.where(np.isfinite(hif), hif - 1e-9, hif))
    return free, full, (lambda xf: p.f(np, full(xf), d)), (lambda xf: p.jac(np, full(xf), d)[:, free]), lof, hif, s


@pytest.mark.parametrize("name", sorted(L.PROBLEMS))
def test_with_every_bound_infinite_it_is_the_unbounded_restatement_bitwise(name):
    p = L.PROBLEMS[name]
    x0, data, _ = p.members(p.batch)
    for q in range(min(p.batch, 3)):
        d = None if data is None else data[q]
        for dt in (np.float64, L.LD) if p.m * p.n <= 1000 else (np.float64,):
            want = L.solve(p, x0[q], d, dt, **p.options)[0]
            for lo, hi in ((None, None), (np.full(p.n, -B.INF), None)):
                got = B.solve(p, x0[q], d, lo, hi, dt, **p.options)
                for k in L.SCALARS + L.COUNTERS + ("x", "xtrial", "D"):
                    assert np.array_equal(getattr(got, k), getattr(want, k), equal_nan=True), (q, dt, k)
                assert not got.peg.any() and got.clipped == 0 and got.alpha == 1 and got.margin == B.INF


@pytest.mark.parametrize("name", sorted(B.PROBLEMS))
def test_float64_and_longdouble_take_the_same_decisions_and_no_peg_is_within_rounding(name):
    p, x0, data, lo, hi, r64, rld = _runs(name)
    for q, (a, l) in enumerate(zip(r64, rld)):
        assert _decisions(a) == _decisions(l), (q, _decisions(a), _decisions(l))
        assert l.margin > B.MARGIN and a.info == 0 and a.status in (1, 2, 3, 4), (q, l.margin, a.status)
    print(f"\n{name}: {len(r64)} members, status {sorted({a.status for a in r64})}, nfev up to {max(a.nfev for a in r64)}, held at the end "
          f"{[int((a.peg != 0).sum()) for a in r64]}, least margin {min(l.margin for l in rld):.1e}")
    assert any(a.peg.any() for a in r64), "the bounds are active"


@pytest.mark.parametrize("name", sorted(B.KINDS))
def test_bounded_members_end_at_kkt_points_that_scipy_finds(name):
    p, x0, data, lo, hi, r64, rld = _runs(name)
    o = dict(L.DEFAULTS)
    o.update(p.options)
    gcap = max(o["gtol"], float(np.sqrt(o["ftol"])))       # a run that ends by ftol has prered <= ftol, and prered >= gnorm^2
    worst = 0.0
    for q, a in enumerate(r64):
        d = None if data is None else data[q]
        x = np.asarray(a.x, dtype=np.float64)
        assert np.all(x >= lo[q]) and np.all(x <= hi[q]), q
        assert np.array_equal(x[a.peg == -1], lo[q][a.peg == -1]) and np.array_equal(x[a.peg == 1], hi[q][a.peg == 1]), q
        assert float(a.gnorm) <= gcap, (q, float(a.gnorm))
        J, f = p.jac(np, x, d), p.f(np, x, d)
        cn = np.linalg.norm(J, axis=0)
        g = (J.T @ f) / np.where(cn == 0, 1.0, cn) / np.linalg.norm(f)          # the scaled gradient at the final x
        atlo, athi = x == lo[q], x == hi[q]
        inside = ~atlo & ~athi
        assert np.all(np.abs(g[inside]) <= 2 * gcap), (q, g)
        assert np.all(g[atlo & ~athi] >= -2 * gcap) and np.all(g[athi & ~atlo] <= 2 * gcap), (q, g)
        assert np.all(g[a.peg == -1] > -2 * gcap) and np.all(g[a.peg == 1] < 2 * gcap), (q, g, a.peg)
        free, full, fun, jac, lof, hif, s = _free_problem(p, x0[q], d, lo[q], hi[q])
        res = scipy_optimize.least_squares(fun, s, jac=jac, bounds=(lof, hif), method="trf", ftol=1e-14, xtol=1e-14, gtol=1e-14, max_nfev=5000)
        xs = full(res.x)
        worst = max(worst, float(np.linalg.norm(x - xs) / np.linalg.norm(xs)))
    print(f"\n{name}: worst |x - x_trf| / |x_trf| {worst:.2e} (cap {TRF_CAP:.2e})")
    assert worst <= TRF_CAP


@pytest.mark.parametrize("name", sorted(n for n in B.PROBLEMS if n.startswith("linbox")))
def test_linear_members_agree_with_bvls(name):
    p, x0, data, lo, hi, r64, rld = _runs(name)
    worst = 0.0
    for q, a in enumerate(r64):
        A, b = p.split(np, data[q])
        fixed = lo[q] == hi[q]
        res = scipy_optimize.lsq_linear(A[:, ~fixed], b - A[:, fixed] @ lo[q][fixed], bounds=(lo[q][~fixed], hi[q][~fixed]), method="bvls",
                                        tol=1e-15)
        xs = np.array(lo[q])
        xs[~fixed] = res.x
        x = np.asarray(a.x, dtype=np.float64)
        assert np.array_equal(x[fixed], lo[q][fixed]), "a fixed parameter never moves"
        worst = max(worst, float(np.linalg.norm(x - xs) / np.linalg.norm(xs)))
    print(f"\n{name}: worst |x - x_bvls| / |x_bvls| {worst:.2e} (cap {BVLS_CAP:.2e})")
    assert worst <= BVLS_CAP


def test_bad_bounds_and_a_start_outside_the_box():
    x0 = np.array([1.0, 2.0])
    for lo, hi in (([2.0, 0.0], [1.0, 3.0]), ([np.nan, 0.0], None), (None, [3.0, np.nan]), ([1.5, 0.0], None), (None, [3.0, 1.0])):
        mem = B.BMember(x0, lo, hi)
        assert mem.info == -2 and not mem.running()
    assert B.BMember(x0, [1.0, 2.0], [1.0, 2.0]).running()                     # every parameter fixed: a box, and x0 inside it


def test_a_member_whose_every_column_is_held_ends_with_status_4():
    p = B.PROBLEMS["linbox16x3"]
    x0, data, lo, hi = p.members(1)
    mem = B.solve(p, lo[0].copy(), data[0], lo[0], lo[0])                      # every parameter fixed at lo
    assert (mem.status, mem.nfev, mem.njev) == (4, 1, 1) and np.array_equal(mem.x, lo[0]) and float(mem.gnorm) == 0.0


def test_peg_sum_is_the_kernels_order():
    rng = np.random.default_rng(8)
    for m in (1, 63, 64, 65, 200):
        a, b = rng.standard_normal(m), rng.standard_normal(m)
        got = B.peg_sum(a, b)
        assert abs(got - float(np.dot(a.astype(L.LD), b.astype(L.LD)))) <= 2 * m * L.EPS * np.linalg.norm(a) * np.linalg.norm(b)
    a, b = np.zeros(65), np.zeros(65)                                         # rows 0 and 64 meet in lane 0: -1, then one fma on top of it
    a[0], b[0], a[64], b[64] = 1.0, -1.0, 1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30
    assert B.peg_sum(a, b) == 2.0 ** -29 + 2.0 ** -60
