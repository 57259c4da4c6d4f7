"""-m gpu: batched robust and weighted least squares (mi355x_qr.h section 8j), member by member.

Shapes, the planted inputs, the restatement of the method and the measures: tests/batched_irls_ref.py.  The shapes cover the wave route
(its smallest member, each register width, both of its edges m == 64 and n + 1 == 32) and the workgroup route (the first shapes past each
edge, qr_irls_batched_max_rows(63) rows).  Every buffer has an odd stride larger than packed (A an odd leading dimension too), a base one
element off, and is sentinel-filled outside its blocks; nothing outside the blocks may change and the inputs may not change at all.
Batches are 9, 5 and 1.

Asserted on every member of the planted inputs at tol = 1e-6, Huber and (where m >= 2 n) bisquare: info == 0; the solve count and the
status of the float64 restatement, no exception (tests/test_batched_irls_ref.py holds every deciding change 1 % away from tol); the three
measures (x, s, w against the longdouble restatement run for the same number of solves) each <= min(4 max(the same measure of the
float64 restatement, eps / 4), cap), cap = 50 kappa eps; and on the shapes with m >= 4 n and m >= 32 the recovery conditions.  A case that
exceeds 4 x on the GPU is listed in MEASURED with its measured ratio and bounded at twice that (five are: x on the smallest shapes, all
below 4 eps); the cap holds for it all the same.  The ratios are printed (-s) and tabulated in DESIGN.md section 7q.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batched_irls_ref as R
import hp_ref as H

pytestmark = pytest.mark.gpu

EPS = R.EPS
SENTINEL = -7.25e33
ISENT = 77
BATCH = R.BATCH
LS, HUBER, BISQUARE = R.LS, R.HUBER, R.BISQUARE

# (m, n, loss, measure) -> the ratio to the float64 restatement (floored at eps / 4, as in the rule) measured on an MI355X where it exceeds
# 4; the bound of such a case is twice the ratio, and never above the cap
# (all five are x on the smallest shapes, where the float64 restatement happens to end within half an eps of the longdouble one and the
# kernels within 4 eps: 8.6e-16, 4.7e-16, 6.0e-16, 5.8e-16 and 8.4e-16)
MEASURED = {(3, 2, HUBER, "x"): 4.03, (8, 2, HUBER, "x"): 4.35, (8, 2, BISQUARE, "x"): 10.86, (16, 7, HUBER, "x"): 5.48,
            (16, 7, BISQUARE, "x"): 6.11}

# the shapes of the exact-property and special-member tests: both routes, each register width of the wave route
EXACT = [(3, 2), (16, 7), (64, 15), (64, 31), (65, 15), (40, 32), (100, 20)]
SPECIAL = [(16, 7), (64, 31), (40, 32), (100, 20)]
TIGHT = [(64, 15, HUBER), (100, 20, BISQUARE)]


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


def _odd(x):
    return x + 3 - x % 2


class Strided:
    """`batch` column-major blocks of rows x cols at an odd leading dimension > rows and an odd stride > ld * cols, the base one
    element off; everything outside the blocks holds the sentinel"""

    def __init__(self, rows, cols, batch, fill=None, dtype=np.float64):
        self.shape = (batch, rows, cols)
        self.ld = _odd(rows)
        self.stride = _odd(self.ld * cols + 4)
        self.init = np.full(1 + batch * self.stride, SENTINEL if dtype == np.float64 else ISENT, dtype=dtype)
        if fill is not None:
            self.view(self.init)[...] = fill
        self.t = torch.from_numpy(self.init.copy()).cuda()
        torch.cuda.synchronize()
        self.ptr = self.t[1:]

    def view(self, flat):
        b, r, c = self.shape
        s = flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[1:], shape=(b, r, c), strides=(s * self.stride, s, s * self.ld))

    def get(self):
        """the blocks as a (batch, rows, cols) array; asserts that nothing outside them changed"""
        torch.cuda.synchronize()
        flat = self.t.cpu().numpy()
        mask = np.ones(flat.shape, dtype=bool)
        self.view(mask)[...] = False
        assert np.array_equal(flat[mask], self.init[mask]), "written outside the blocks"
        return self.view(flat).copy()

    def unchanged(self):
        torch.cuda.synchronize()
        return np.array_equal(self.t.cpu().numpy(), self.init, equal_nan=True)


ALL = ("w", "scale", "resid", "iter", "status")
KEYS = ("X", "W", "scale", "resid", "iter", "status", "info")


def _solve(plan, loss, A, b, prior=None, shared=False, scale=None, x0=None, tol=R.TOL, maxit=0, tune=0.0, want=ALL):
    """one qr_irls_batched_dev call on members A (batch, m, n), b (batch, m); prior: None (a NULL pointer), (batch, m), or with
    shared=True (m,) passed with stride 0; scale: None or (batch,); x0: None or (batch, n)"""
    bt, m, n = A.shape
    dA, dB = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None])
    nb = 1 if shared else bt
    dP = None if prior is None else Strided(m, 1, nb, np.reshape(prior, (nb, m, 1)))
    dX0 = None if x0 is None else Strided(n, 1, bt, np.reshape(x0, (bt, n, 1)))
    dS = None if scale is None else torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float64)).cuda()
    dX, dW = Strided(n, 1, bt), Strided(m, 1, bt)
    dsc = torch.full((bt + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    dres = torch.full((bt + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    dit = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    dst = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    dinfo = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(tune=tune, tol=tol, maxit=maxit, strideprior=0 if shared else dW.stride)       # (the prior buffers have dW's geometry)
    if dP is not None:
        kw.update(dprior=dP.ptr)
    if dS is not None:
        kw.update(dscale_in=dS)
    if dX0 is not None:
        kw.update(dX0=dX0.ptr, strideX0=dX0.stride)
    if "w" in want:
        kw.update(dW=dW.ptr, strideW=dW.stride)
    if "scale" in want:
        kw.update(dscale=dsc[1:])
    if "resid" in want:
        kw.update(dresid=dres[1:])
    if "iter" in want:
        kw.update(diter=dit[1:])
    if "status" in want:
        kw.update(dstatus=dst[1:])
    plan.irls_batched(loss, dA.ptr, m, n, dA.ld, dA.stride, dB.ptr, dB.stride, dX.ptr, dX.stride, dinfo[1:], bt, **kw)
    plan.sync()
    for buf in (dA, dB, dP, dX0):
        assert buf is None or buf.unchanged(), "the inputs and their padding are untouched"
    if "w" not in want:
        assert dW.unchanged()
    sc, res, it, st, info = dsc.cpu().numpy(), dres.cpu().numpy(), dit.cpu().numpy(), dst.cpu().numpy(), dinfo.cpu().numpy()
    for v, s in ((sc, SENTINEL), (res, SENTINEL), (it, ISENT), (st, ISENT), (info, ISENT)):
        assert v[0] == s and v[-1] == s
    for name, v, s in (("scale", sc, SENTINEL), ("resid", res, SENTINEL), ("iter", it, ISENT), ("status", st, ISENT)):
        if name not in want:
            assert np.all(v == s)
    return dict(X=dX.get()[:, :, 0], W=dW.get()[:, :, 0], scale=sc[1:-1], resid=res[1:-1], iter=it[1:-1], status=st[1:-1], info=info[1:-1])


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _within(tag, key, got, ref, cap):
    factor = 2.0 * MEASURED[key] if key in MEASURED else 4.0
    bound = min(factor * max(ref, EPS / 4), cap)             # (factor 4: min(4 max(ref, eps / 4), cap), the rule)
    print(f"RATIO {tag}: {got:.3e} is {got / max(ref, EPS / 4):.2f} x the float64 reference {ref:.3e}; bound {bound:.3e} (cap {cap:.3e})")
    assert np.isfinite(got) and got <= bound, (tag, got, ref, bound)


def _gels(plan, A, b):
    """qr_gels_batched_dev's x of packed members"""
    bt, m, n = A.shape
    dA = torch.from_numpy(np.ascontiguousarray(A.transpose(0, 2, 1))).cuda()
    dB = torch.from_numpy(np.array(b, dtype=np.float64)).cuda()
    tau = torch.zeros(bt * n, dtype=torch.float64, device="cuda")
    ginfo = torch.zeros(bt, dtype=torch.int32, device="cuda")
    plan.gels_batched(dA, m, n, m, m * n, tau, n, dB, 1, m, m, ginfo, bt)
    plan.sync()
    assert np.all(ginfo.cpu().numpy() == 0)
    return dB.cpu().numpy().reshape(bt, m)[:, :n].copy()


# ------------------------------------------------------------------------------------------------
# the planted inputs, every shape
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", R.SHAPES)
def test_planted_members_counts_accuracy_and_recovery(plan, qr, m, n):
    assert bool(qr.lib.qrd_ir_wave_route(m, n)) == ((m, n) in R.WAVE_SHAPES)
    assert m <= qr.irls_batched_max_rows(n)
    fails = []
    for loss in R.losses(m, n):
        name = R.LOSS_NAMES[loss]
        c = R.case(m, n, loss)
        out = _solve(plan, loss, c["A"], c["b"])
        assert np.all(out["info"] == 0), out["info"]
        it64 = np.array([o["iter"] for o in c["out64"]])
        st64 = np.array([o["status"] for o in c["out64"]])
        print(f"COUNTS irls {m}x{n} {name}: device {list(out['iter'])} status {list(out['status'])}; restatement {list(it64)} status {list(st64)}")
        assert np.array_equal(out["iter"], it64) and np.array_equal(out["status"], st64)
        worst = [0.0] * 3
        xls = None
        if R.recovers(m, n):
            ls = _solve(plan, LS, c["A"], c["b"])
            assert np.all(ls["info"] == 0) and np.all(ls["iter"] == 1) and np.all(ls["status"] == 0)
            xls = ls["X"]
        for q in range(BATCH):
            A, b = c["A"][q], c["b"][q]
            got = R.measures(A, b, out["X"][q], out["scale"][q], out["W"][q], c["outld"][q])
            rl = H.arr(b) - H.matmul(H.arr(A), H.arr(out["X"][q])[:, None])[:, 0]
            nrm = float(H.norm(A)) * float(H.norm(out["X"][q])) + float(H.norm(b))
            assert abs(out["resid"][q] - float(H.norm(rl))) <= (n + 4) * EPS * nrm, (q, "resid")      # (n fused terms per row)
            for k, mname in enumerate(R.NAMES):
                ref = c["ref"][q][k]
                worst[k] = max(worst[k], got[k] / max(ref, EPS / 4))
                try:
                    _within(f"irls {m}x{n} {name} member {q} {mname}", (m, n, loss, mname), got[k], ref, c["cap"][q])
                except AssertionError as e:
                    fails.append(e.args[0])
            if R.recovers(m, n):
                rows, xs = c["rows"][q], c["xstar"][q]
                ratio = R.scaled_error(A, out["X"][q], xs) / R.scaled_error(A, xls[q], xs)
                assert ratio < 0.5, (name, q, ratio)
                if loss == HUBER:
                    assert np.all(out["W"][q][rows] < 0.5), (q, out["W"][q][rows])
                else:
                    assert np.all(out["W"][q][rows] == 0.0), (q, out["W"][q][rows])
        print(f"WORST irls {m}x{n} {name}: " + ", ".join(f"{mn} {w:.2f} x" for mn, w in zip(R.NAMES, worst)) + " the float64 reference; "
              f"solves mean {np.mean(out['iter']):.1f} max {np.max(out['iter'])}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------
# exact properties, bitwise
# ------------------------------------------------------------------------------------------------
def _loss_of(m, n):
    return BISQUARE if (m >= 2 * n and (m + n) % 2 == 0) else HUBER


@pytest.mark.parametrize("m,n", EXACT)
def test_repeatable_and_independent_of_batch_index_and_optional_outputs(plan, m, n):
    loss = _loss_of(m, n)
    c = R.case(m, n, loss)
    A, b = c["A"], c["b"]
    rng = np.random.default_rng(m * 100 + n)
    prior = rng.uniform(0.5, 2.0, (BATCH, m))
    if m > 2 * n:
        prior[:, m // 2] = 0.0
    full = _solve(plan, loss, A, b, prior)
    assert np.all(full["info"] == 0)
    assert _same(full, _solve(plan, loss, A, b, prior)), "repeated calls are equal"
    perm = [7, 2, 8, 0, 4]
    sub = _solve(plan, loss, A[perm], b[perm], prior[perm])   # batch 5: a workgroup of the wave route that is not full
    for k in KEYS:
        assert np.array_equal(sub[k], full[k][perm]), k
    one = _solve(plan, loss, A[[3]], b[[3]], prior[[3]])      # batch 1
    for k in KEYS:
        assert np.array_equal(one[k], full[k][[3]]), k
    bare = _solve(plan, loss, A, b, prior, want=())
    assert np.array_equal(bare["X"], full["X"]) and np.array_equal(bare["info"], full["info"])
    some = _solve(plan, loss, A[perm], b[perm], prior[perm], want=("w", "iter"))
    assert np.array_equal(some["X"], full["X"][perm]) and np.array_equal(some["W"], full["W"][perm])
    assert np.array_equal(some["iter"], full["iter"][perm])
    # one weight vector for all members (stride 0) against per-member copies of it
    p0 = prior[4].copy()
    tiled = _solve(plan, loss, A, b, np.tile(p0, (BATCH, 1)))
    assert _same(tiled, _solve(plan, loss, A, b, p0, shared=True)), "shared weights equal per-member copies"
    # no weights at all against ones
    assert _same(_solve(plan, loss, A, b), _solve(plan, loss, A, b, np.ones((BATCH, m)))), "a NULL dprior is ones"


@pytest.mark.parametrize("m,n", EXACT)
def test_scaling_by_powers_of_two_is_exact(plan, m, n):
    loss = _loss_of(m, n)
    c = R.case(m, n, loss)
    idx = [0, 1, 2, 3, 4]                                     # batch 5: plain and graded members
    A, b = c["A"][idx], c["b"][idx]
    base = _solve(plan, loss, A, b)
    assert np.all(base["info"] == 0)
    for e in (20, -20):
        s = 2.0 ** e
        out = _solve(plan, loss, s * A, s * b)                # (A, b) scaled: the same x, w, count and status; s and resid by the factor
        assert _same(out, base, ("X", "W", "iter", "status", "info"))
        assert np.array_equal(out["scale"], s * base["scale"]) and np.array_equal(out["resid"], s * base["resid"])
    for e in (7, -5):
        s = 2.0 ** e
        out = _solve(plan, loss, A, s * b)                    # b scaled: x, s and resid scale exactly
        assert np.array_equal(out["X"], s * base["X"]) and np.array_equal(out["scale"], s * base["scale"])
        assert np.array_equal(out["resid"], s * base["resid"]) and _same(out, base, ("W", "iter", "status", "info"))


# ------------------------------------------------------------------------------------------------
# special members beside unaffected neighbours
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SPECIAL)
def test_least_squares_loss_weights_and_masks_bitwise(plan, qr, m, n):
    c = R.members(m, n, salt=1)
    A, b = c["A"], c["b"]
    # no weights: qr_gels_batched_dev's x, bitwise, on the same route
    xg = _gels(plan, A, b)
    ls = _solve(plan, LS, A, b)
    assert np.all(ls["info"] == 0) and np.array_equal(ls["X"], xg), "QR_LOSS_LS with NULL weights is qr_gels_batched_dev"
    assert np.all(ls["iter"] == 1) and np.all(ls["status"] == 0) and np.all(ls["W"] == 1.0) and np.all(ls["scale"] == 0.0)
    # weights that are powers of 4: the plain call on rows scaled by the powers of 2
    rng = np.random.default_rng(m + n)
    e = rng.integers(-3, 4, (BATCH, m))
    w4 = _solve(plan, LS, A, b, 4.0 ** e)
    f = 2.0 ** e
    assert np.array_equal(w4["X"], _gels(plan, A * f[:, :, None], b * f)), "weights 4^e are rows scaled by 2^e"
    for q in range(BATCH):                                    # resid is unweighted
        assert abs(w4["resid"][q] - np.linalg.norm(b[q] - A[q] @ w4["X"][q])) <= 1e-12 * np.linalg.norm(b[q])
    # a masked row that holds NaN is a masked row that holds zeros, under every loss
    p = rng.uniform(0.5, 2.0, (BATCH, m))
    mask = [0, m // 2] if m > n + 1 else [0]
    p[:, mask] = 0.0
    An, bn, Az, bz = A.copy(), b.copy(), A.copy(), b.copy()
    An[:, mask, :], bn[:, mask] = np.nan, np.nan
    Az[:, mask, :], bz[:, mask] = 0.0, 0.0
    for loss in (LS,) + R.losses(m, n):
        on, oz = _solve(plan, loss, An, bn, p), _solve(plan, loss, Az, bz, p)
        assert np.all(on["info"] == 0) and _same(on, oz), R.LOSS_NAMES[loss]
        assert np.all(on["W"][:, mask] == 1.0)
    # the device wrapper of the weighted solve and the Python wrappers
    dA, dB, dP, dX = Strided(m, n, BATCH, An), Strided(m, 1, BATCH, bn[:, :, None]), Strided(m, 1, BATCH, p[:, :, None]), Strided(n, 1, BATCH)
    dinfo = torch.full((BATCH,), ISENT, dtype=torch.int32, device="cuda")
    dres = torch.full((BATCH,), SENTINEL, dtype=torch.float64, device="cuda")
    plan.gels_weighted_batched(dA.ptr, m, n, dA.ld, dA.stride, dB.ptr, dB.stride, dP.ptr, dP.stride, dX.ptr, dX.stride, dinfo, BATCH, dresid=dres)
    plan.sync()
    wl = _solve(plan, LS, An, bn, p)
    assert np.array_equal(dX.get()[:, :, 0], wl["X"]) and np.array_equal(dres.cpu().numpy(), wl["resid"]) and np.all(dinfo.cpu().numpy() == 0)
    Xw, rw, fw = qr.lstsq_weighted_batched(An, bn, p)
    assert np.array_equal(Xw, wl["X"]) and np.array_equal(rw, wl["resid"]) and np.all(fw == 0)


@pytest.mark.parametrize("m,n", SPECIAL)
def test_special_members_and_their_neighbours(plan, qr, m, n):
    c = R.members(m, n, salt=2)
    A, b = c["A"].copy(), c["b"].copy()
    prior = np.ones((BATCH, m))
    jz = n // 2
    prior[1][m - 1] = -1.0                                    # a negative weight
    prior[3][0] = np.nan                                      # a NaN weight
    prior[5][m // 2] = np.inf                                 # an infinite weight
    A[4][:, jz] = 0.0                                         # an exactly zero column: jz + 1
    prior[6][:] = 0.0
    prior[6][:n - 1] = 1.0                                    # fewer than n rows of positive weight
    b[7][:] = 0.0                                             # an exact fit: x = 0, s = 0, status 2
    want = np.zeros(BATCH, dtype=np.int32)
    want[[1, 3, 5]] = -1
    want[4] = jz + 1
    want[6] = -2
    bad = [1, 3, 4, 5, 6]
    good = [q for q in range(BATCH) if q not in bad]
    out = _solve(plan, HUBER, A, b, prior)
    assert np.array_equal(out["info"], want), out["info"]
    for q in bad:                                             # nothing but info is written
        assert np.all(out["X"][q] == SENTINEL) and np.all(out["W"][q] == SENTINEL) and out["scale"][q] == SENTINEL
        assert out["resid"][q] == SENTINEL and out["iter"][q] == ISENT and out["status"][q] == ISENT
    alone = _solve(plan, HUBER, A[good], b[good], prior[good])
    assert np.all(alone["info"] == 0)
    for k in KEYS:
        assert np.array_equal(out[k][good], alone[k]), k
    assert out["status"][7] == 2 and out["iter"][7] == 1 and np.all(out["X"][7] == 0.0) and np.all(out["W"][7] == 1.0)
    assert out["scale"][7] == 0.0 and out["resid"][7] == 0.0
    for q in (0, 2, 8):
        ref = R.irls(A[q], b[q], HUBER, tol=R.TOL)
        assert out["status"][q] == ref["status"] and abs(int(out["iter"][q]) - ref["iter"]) <= 1, q
        assert R.scaled_error(A[q], out["X"][q], ref["x"]) <= 1e-5 and np.max(np.abs(out["W"][q] - ref["w"])) <= 1e-2
    # the host twin and the Python wrapper: the same members, zeros where nothing was computed; the wrapper does not raise
    Xw, ww, sw, rw, iw, tw, fw = qr.lstsq_robust_batched(A, b, "huber", weights=prior, tol=R.TOL)
    assert np.array_equal(fw, want)
    assert np.array_equal(Xw[good], alone["X"]) and np.array_equal(ww[good], alone["W"]) and np.array_equal(sw[good], alone["scale"])
    assert np.array_equal(rw[good], alone["resid"]) and np.array_equal(iw[good], alone["iter"]) and np.array_equal(tw[good], alone["status"])
    for q in bad:
        assert np.all(Xw[q] == 0.0) and np.all(ww[q] == 0.0) and sw[q] == 0.0 and rw[q] == 0.0 and iw[q] == 0 and tw[q] == 0
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    X = np.full((BATCH, n), 3.0)
    info = np.full(BATCH, ISENT, dtype=np.intc)
    At = np.ascontiguousarray(A.transpose(0, 2, 1))
    rc = qr.lib.qr_lstsq_robust_batched(At.ctypes.data_as(dp), m, n, np.ascontiguousarray(b).ctypes.data_as(dp), HUBER, 0.0,
                                        np.ascontiguousarray(prior).ctypes.data_as(dp), None, None, R.TOL, 0, BATCH, X.ctypes.data_as(dp), None,
                                        None, None, None, None, info.ctypes.data_as(ip))
    assert rc == qr.QR_E_SINGULAR and np.array_equal(info, want) and np.array_equal(X[good], alone["X"])


@pytest.mark.parametrize("m,n", SPECIAL)
def test_fixed_scale_warm_start_and_the_count(plan, m, n):
    loss = BISQUARE if m >= 2 * n else HUBER
    c = R.case(m, n, loss)
    A, b = c["A"], c["b"]
    conv = _solve(plan, loss, A, b, tol=1e-10, maxit=200)
    assert np.all(conv["info"] == 0)
    done = np.flatnonzero(conv["status"] == 0)                # (a member may cycle at this tolerance: the MAD scale moves with the iterate)
    assert len(done) >= BATCH // 2 and np.all(conv["status"][conv["status"] != 0] == 3)
    # a warm start from the converged x: one solve, status 0
    warm = _solve(plan, loss, A, b, x0=conv["X"])
    assert np.all(warm["info"] == 0) and np.all(warm["iter"][done] == 1) and np.all(warm["status"][done] == 0)
    for q in done:
        assert R.scaled_error(A[q], warm["X"][q], conv["X"][q]) <= R.TOL
    # a Huber fit as the start of a bisquare fit
    if loss == BISQUARE:
        hub = _solve(plan, HUBER, A, b)
        cold, hot = _solve(plan, BISQUARE, A, b), _solve(plan, BISQUARE, A, b, x0=hub["X"])
        assert np.all(hot["info"] == 0) and np.all(hot["status"] == 0)         # (the loss is not convex: the two fits may differ)
        for q in range(BATCH):
            assert R.scaled_error(A[q], hot["X"][q], cold["X"][q]) <= 0.05, q
    # a fixed scale: returned as given; the weights are those of the returned x at that scale (Huber below m = 4 n: from a cold start a
    # bisquare fit at a fixed scale can lose its weights there, which ends with info -2, as the restatement's does)
    fl = loss if R.recovers(m, n) else HUBER
    sfix = 1.5 * conv["scale"]
    sfix[2] = 0.0                                             # no scale
    sfix[5] = np.nan
    sfix[6] = np.inf
    sfix[8] = -conv["scale"][8]
    fx = _solve(plan, fl, A, b, scale=sfix)
    bad = [2, 5, 6, 8]
    good = [q for q in range(BATCH) if q not in bad]
    assert np.all(fx["info"][bad] == -1) and np.all(fx["info"][good] == 0)
    for q in bad:
        assert np.all(fx["X"][q] == SENTINEL) and np.all(fx["W"][q] == SENTINEL) and fx["scale"][q] == SENTINEL and fx["iter"][q] == ISENT
    alone = _solve(plan, fl, A[good], b[good], scale=sfix[good])
    for k in KEYS:
        assert np.array_equal(fx[k][good], alone[k]), k
    k = R.DEFAULT_TUNE[fl]
    for q in good:
        assert fx["scale"][q] == sfix[q] and fx["status"][q] in (0, 3)
        r = np.asarray(R.residual(A[q], b[q], fx["X"][q]), dtype=np.float64)
        wref = R.weight(fl, np.abs(r) / sfix[q], k)
        assert np.max(np.abs(fx["W"][q] - wref)) <= 1e-9, q
        ref = R.irls(A[q], b[q], fl, scale=sfix[q], tol=R.TOL)
        assert ref["info"] == 0 and ref["status"] == fx["status"][q] and abs(ref["iter"] - int(fx["iter"][q])) <= 1, q
        assert R.scaled_error(A[q], fx["X"][q], ref["x"]) <= 1e-5, q
    # a bisquare member whose warm start and tiny fixed scale zero every weight: info -2 beside unaffected neighbours
    if loss == BISQUARE:
        tiny = conv["scale"].copy()
        tiny[4] = 1e-12 * conv["scale"][4]
        x0 = conv["X"]
        zz = _solve(plan, BISQUARE, A, b, scale=tiny, x0=x0, maxit=3)
        assert zz["info"][4] == -2 and np.all(zz["X"][4] == SENTINEL) and zz["iter"][4] == ISENT
        rest = [q for q in range(BATCH) if q != 4]
        assert np.all(zz["info"][rest] == 0)
        z2 = _solve(plan, BISQUARE, A[rest], b[rest], scale=tiny[rest], x0=x0[rest], maxit=3)
        for kk in KEYS:
            assert np.array_equal(zz[kk][rest], z2[kk]), kk
    # maxit = 1: status 3 after one solve, with x (the least-squares solution), w and s written
    k = R.DEFAULT_TUNE[loss]
    cut = _solve(plan, loss, A, b, maxit=1)
    full = R.case(m, n, loss)["out64"]
    ls = _solve(plan, LS, A, b)
    for q in range(BATCH):
        assert cut["info"][q] == 0 and cut["iter"][q] == 1
        assert cut["status"][q] == (3 if full[q]["iter"] > 1 else full[q]["status"])
        assert np.array_equal(cut["X"][q], ls["X"][q]) and cut["resid"][q] == ls["resid"][q]
        r = np.asarray(R.residual(A[q], b[q], cut["X"][q]), dtype=np.float64)
        s = np.median(np.abs(r)) / R.MAD
        assert abs(cut["scale"][q] - s) <= 1e-9 * s and np.max(np.abs(cut["W"][q] - R.weight(loss, np.abs(r) / s, k))) <= 1e-6


def test_one_by_one_and_exact_fits_leave_with_status_two(plan):
    A = np.array([[[2.0]], [[-4.0]], [[0.5]]])
    b = np.array([[3.0], [1.0], [0.0]])
    for loss in (HUBER, BISQUARE):
        o = _solve(plan, loss, A, b)
        assert np.all(o["info"] == 0) and np.all(o["status"] == 2) and np.all(o["iter"] == 1)
        assert np.array_equal(o["X"][:, 0], [1.5, -0.25, 0.0]) and np.all(o["W"] == 1.0) and np.all(o["scale"] == 0.0) and np.all(o["resid"] == 0.0)
    z = _solve(plan, HUBER, np.zeros((1, 1, 1)), np.ones((1, 1)))
    assert z["info"][0] == 1 and z["X"][0, 0] == SENTINEL
    # more than half the rows fitted exactly, both routes: the top of A is a diagonal of powers of two, the rows below are zeros
    for m, n in ((9, 4), (70, 33)):
        Am = np.zeros((1, m, n))
        Am[0, :n, :n] = np.diag(2.0 ** (np.arange(n) % 5 - 2))
        bm = np.zeros((1, m))
        bm[0, :n] = np.arange(1, n + 1) * 0.375
        bm[0, m - 1] = 7.0                                    # one row that nothing fits
        o = _solve(plan, BISQUARE, Am, bm)
        assert o["info"][0] == 0 and o["status"][0] == 2 and o["iter"][0] == 1 and o["scale"][0] == 0.0 and o["resid"][0] == 7.0
        assert np.array_equal(o["X"][0], bm[0, :n] / np.diag(Am[0, :n, :n])) and np.all(o["W"] == 1.0)


@pytest.mark.parametrize("m,n,loss", TIGHT)
def test_tight_tolerance_reaches_the_estimating_equation(plan, m, n, loss):
    c = R.case(m, n, loss)
    idx = [0, 1, 2, 3, 4]
    A, b = c["A"][idx], c["b"][idx]
    out = _solve(plan, loss, A, b, tol=1e-12, maxit=200)
    assert np.all(out["info"] == 0)
    one = np.ones(m)
    for q in range(len(idx)):
        ref = R.irls(A[q], b[q], loss, tol=1e-12, maxit=200)
        got = R.estimating_equation(A[q], one, out["W"][q], out["X"][q], b[q])
        want = R.estimating_equation(A[q], one, ref["w"], ref["x"], b[q])
        print(f"ESTIMATING irls {m}x{n} {R.LOSS_NAMES[loss]} member {q}: {got:.3e} after {out['iter'][q]} solves (status {out['status'][q]}); "
              f"the float64 restatement {want:.3e} after {ref['iter']} (status {ref['status']})")
        assert got <= 4 * want, (q, got, want)
