"""-m gpu: batched bound-constrained least squares (mi355x_qr.h section 8i), member by member.

Shapes, the planted inputs, the restatement of the method and the measures: tests/batched_bvls_ref.py.  The shapes cover the wave route
(its smallest member, each register width, both of its edges m == 64 and n + 1 == 32) and the workgroup route (the first shapes past each
edge, m == n at full width, qr_bvls_batched_max_rows(63) rows).  Every buffer has an odd stride larger than packed (A an odd leading
dimension too), a base one element off, and is sentinel-filled outside its blocks; nothing outside the blocks may change and the inputs
may not change at all.  Batches are 9, 5 and 1.

Asserted on every member of the planted inputs: info == 0, the planted state exactly, bound variables bitwise on their bounds and
lo <= x <= hi with no tolerance, the sign of w on every bound variable, iter <= 3 n, and the three measures (stationarity over the free
variables, w, resid) within the rule of test_gpu_range_edges.py: each <= min(max(4 x the same measure of the float64 restatement on the
same input, eps), cap), cap = (m + n) eps.  A case that exceeds 4 x on the GPU would be listed in MEASURED at twice its measured ratio; the
cap holds for it all the same.  The ratios, the forward errors and the iteration counts are printed (-s) and tabulated in DESIGN.md
section 7p; the forward error is not asserted (it depends on kappa^2 ||r||).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batched_bvls_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
INF = np.inf
SENTINEL = -7.25e33
ISENT = 77
BATCH = R.BATCH

# (m, n, measure) -> the ratio to the float64 restatement (floored at eps / 4, as in the rule) measured on an MI355X where it exceeds 4
# (DESIGN.md section 7p); the bound of such a case is twice the ratio, and never above the cap
MEASURED = {}

# the shapes of the exact-property and special-member tests: both routes, each register width of the wave route, m == n at full width
EXACT = [(2, 2), (8, 7), (16, 15), (64, 31), (65, 31), (100, 33), (63, 63)]
SPECIAL = [(16, 7), (64, 31), (40, 32), (130, 63)]


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


def _solve(plan, A, b, lo, hi, maxit=0, shared=False, want=("w", "state", "resid", "iter")):
    """one qr_bvls_batched_dev call on members A (batch, m, n), b (batch, m); lo / hi: None (a NULL pointer), (batch, n), or with
    shared=True (n,) passed with stride 0"""
    bt, m, n = A.shape
    dA, dB = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None])
    nb = 1 if shared else bt
    dlo = None if lo is None else Strided(n, 1, nb, np.reshape(lo, (nb, n, 1)))
    dhi = None if hi is None else Strided(n, 1, nb, np.reshape(hi, (nb, n, 1)))
    dX, dW, dst = Strided(n, 1, bt), Strided(n, 1, bt), Strided(n, 1, bt, dtype=np.int32)
    dres = torch.full((bt + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    dit = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    dinfo = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(maxit=maxit, stridebnd=0 if shared else dX.stride)                   # (the bound buffers have dX's geometry)
    if dlo is not None:
        kw.update(dlo=dlo.ptr)
    if dhi is not None:
        kw.update(dhi=dhi.ptr)
    if "w" in want:
        kw.update(dW=dW.ptr, strideW=dW.stride)
    if "state" in want:
        kw.update(dstate=dst.ptr, stridestate=dst.stride)
    if "resid" in want:
        kw.update(dresid=dres[1:])
    if "iter" in want:
        kw.update(diter=dit[1:])
    plan.bvls_batched(dA.ptr, m, n, dA.ld, dA.stride, dB.ptr, dB.stride, dX.ptr, dX.stride, dinfo[1:], bt, **kw)
    plan.sync()
    for buf in (dA, dB, dlo, dhi):
        assert buf is None or buf.unchanged(), "the inputs and their padding are untouched"
    if "w" not in want:
        assert dW.unchanged()
    if "state" not in want:
        assert dst.unchanged()
    res, it, info = dres.cpu().numpy(), dit.cpu().numpy(), dinfo.cpu().numpy()
    assert res[0] == SENTINEL and res[-1] == SENTINEL and it[0] == ISENT and it[-1] == ISENT and info[0] == ISENT and info[-1] == ISENT
    if "resid" not in want:
        assert np.all(res == SENTINEL)
    if "iter" not in want:
        assert np.all(it == ISENT)
    return dict(X=dX.get()[:, :, 0], W=dW.get()[:, :, 0], state=dst.get()[:, :, 0], resid=res[1:-1], iter=it[1:-1], info=info[1:-1])


def _case_solve(plan, c, idx=None, **kw):
    idx = list(range(len(c["A"]))) if idx is None else idx
    return _solve(plan, c["A"][idx], c["b"][idx], c["lo"][idx], c["hi"][idx], **kw)


KEYS = ("X", "W", "state", "resid", "iter", "info")


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _within(tag, key, got, ref, cap):
    factor = 2.0 * MEASURED[key] if key in MEASURED else 4.0
    bound = min(factor * max(ref, EPS / 4), cap)             # (factor 4: min(max(4 ref, eps), cap), the rule)
    print(f"RATIO {tag}: {got:.3e} is {got / max(ref, EPS / 4):.2f} x the float64 reference {ref:.3e}; bound {bound:.3e} (cap {cap:.3e})")
    assert np.isfinite(got) and got <= bound, (tag, got, ref, bound)


def _feasible(out, lo, hi, q):
    x, st = out["X"][q], out["state"][q]
    assert np.all(x >= lo) and np.all(x <= hi), "lo <= x <= hi with no tolerance"
    assert np.array_equal(x[st == -1], lo[st == -1]) and np.array_equal(x[st == 1], hi[st == 1]), "bound variables sit on their bounds"
    assert np.all(np.isin(st, (-1, 0, 1)))


# ------------------------------------------------------------------------------------------------
# the planted inputs, every shape
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", R.SHAPES)
def test_planted_members_state_feasibility_and_accuracy(plan, qr, m, n):
    assert bool(qr.lib.qrd_bv_wave_route(m, n)) == ((m, n) in R.WAVE_SHAPES)
    assert m <= qr.bvls_batched_max_rows(n)
    c = R.case(m, n)
    out = _case_solve(plan, c)
    assert np.all(out["info"] == 0), out["info"]
    worst = [0.0] * 3
    fails = []
    fwd, fwd64 = 0.0, 0.0
    for q in range(BATCH):
        assert np.array_equal(out["state"][q], c["state"][q]), (q, "the planted state")
        _feasible(out, c["lo"][q], c["hi"][q], q)
        st = out["state"][q]
        assert np.all(out["W"][q][st == -1] < 0) and np.all(out["W"][q][st == 1] > 0), (q, "the sign of w on the bound variables")
        assert 0 <= out["iter"][q] <= 3 * n
        got = R.measures(c["A"][q], c["b"][q], out["X"][q], out["W"][q], out["resid"][q], st)
        for k, name in enumerate(R.NAMES):
            ref = c["ref"][q][k]
            worst[k] = max(worst[k], got[k] / max(ref, EPS / 4))
            try:
                _within(f"bvls {m}x{n} member {q} {name}", (m, n, name), got[k], ref, c["cap"])
            except AssertionError as e:
                fails.append(e.args[0])
        nx = max(np.linalg.norm(c["xstar"][q]), 1e-300)
        fwd = max(fwd, np.linalg.norm(out["X"][q] - c["xstar"][q]) / nx)
        fwd64 = max(fwd64, np.linalg.norm(np.asarray(c["out64"][q]["x"], dtype=np.float64) - c["xstar"][q]) / nx)
    it64 = [c["out64"][q]["iter"] for q in range(BATCH)]
    print(f"WORST bvls {m}x{n}: " + ", ".join(f"{name} {w:.2f} x" for name, w in zip(R.NAMES, worst)) + " the float64 reference; "
          f"forward error {fwd:.2e} (restatement {fwd64:.2e}); eliminations mean {np.mean(out['iter']):.1f} max {np.max(out['iter'])} "
          f"(restatement mean {np.mean(it64):.1f} max {np.max(it64)}; same counts on {int(np.sum(out['iter'] == np.array(it64)))} of {BATCH})")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------
# exact properties, bitwise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", EXACT)
def test_repeatable_and_independent_of_batch_index_and_optional_outputs(plan, m, n):
    c = R.case(m, n)
    full = _case_solve(plan, c)
    assert _same(full, _case_solve(plan, c)), "repeated calls are equal"
    perm = [7, 2, 8, 0, 4]
    sub = _case_solve(plan, c, perm)                          # batch 5: a workgroup of the wave route that is not full
    for k in KEYS:
        assert np.array_equal(sub[k], full[k][perm]), k
    one = _case_solve(plan, c, [3])                           # batch 1
    for k in KEYS:
        assert np.array_equal(one[k], full[k][[3]]), k
    bare = _case_solve(plan, c, want=())
    assert np.array_equal(bare["X"], full["X"]) and np.array_equal(bare["info"], full["info"])
    some = _case_solve(plan, c, perm, want=("w", "iter"))
    assert np.array_equal(some["X"], full["X"][perm]) and np.array_equal(some["W"], full["W"][perm])
    assert np.array_equal(some["iter"], full["iter"][perm])
    # one bound vector for all members (stride 0) against per-member copies of it
    lo0, hi0 = c["lo"][4].copy(), c["hi"][4].copy()
    tiled = _solve(plan, c["A"], c["b"], np.tile(lo0, (BATCH, 1)), np.tile(hi0, (BATCH, 1)))
    assert _same(tiled, _solve(plan, c["A"], c["b"], lo0, hi0, shared=True)), "shared bounds equal per-member copies"


@pytest.mark.parametrize("m,n", EXACT)
def test_scaling_by_powers_of_two_is_exact(plan, m, n):
    c = R.case(m, n)
    idx = [0, 1, 2, 3, 4]                                     # batch 5: plain and graded members
    A, b, lo, hi = (c[k][idx] for k in ("A", "b", "lo", "hi"))
    base = _solve(plan, A, b, lo, hi)
    assert np.all(base["info"] == 0)
    for e in (20, -20):
        s = 2.0 ** e
        out = _solve(plan, s * A, s * b, lo, hi)              # (A, b) scaled: the same x, state, count; w by s^2, resid by s
        assert _same(out, base, ("X", "state", "iter", "info"))
        assert np.array_equal(out["W"], s * s * base["W"]) and np.array_equal(out["resid"], s * base["resid"])
    for e in (7, -5):
        s = 2.0 ** e
        out = _solve(plan, A, s * b, s * lo, s * hi)          # (b, lo, hi) scaled: x, w and resid scale exactly
        assert np.array_equal(out["X"], s * base["X"]) and np.array_equal(out["W"], s * base["W"])
        assert np.array_equal(out["resid"], s * base["resid"]) and _same(out, base, ("state", "iter", "info"))


# ------------------------------------------------------------------------------------------------
# special members beside unaffected neighbours
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SPECIAL)
def test_special_members_and_their_neighbours(plan, qr, m, n):
    c = R.case(m, n, salt=1)
    A, b, lo, hi = (c[k].copy() for k in ("A", "b", "lo", "hi"))
    jz = n // 2
    lo[1], hi[1] = -INF, INF                                  # all unbounded: one elimination, the plain least-squares solution
    jf = int(np.flatnonzero(c["state"][3] == 0)[0]) if np.any(c["state"][3] == 0) else 0
    lo[3][jf] = hi[3][jf] = 0.125                             # a fixed variable
    lo[2][n - 1], hi[2][n - 1] = 1.0, 0.5                     # lo > hi
    lo[6][0] = np.nan                                         # a NaN bound
    hi[8][jz] = -INF                                          # hi == -inf
    A[5][:, jz] = 0.0                                         # an exactly zero column ...
    lo[5][jz], hi[5][jz] = -INF, INF                          # ... that is free from the start: jz + 1
    want = np.zeros(BATCH, dtype=np.int32)
    want[[2, 6, 8]] = -1
    want[5] = jz + 1
    bad = [2, 5, 6, 8]
    good = [q for q in range(BATCH) if q not in bad]
    out = _solve(plan, A, b, lo, hi)
    assert np.array_equal(out["info"], want), out["info"]
    for q in bad:                                             # nothing but info is written
        assert np.all(out["X"][q] == SENTINEL) and np.all(out["W"][q] == SENTINEL) and np.all(out["state"][q] == ISENT)
        assert out["resid"][q] == SENTINEL and out["iter"][q] == ISENT
    alone = _solve(plan, A[good], b[good], lo[good], hi[good])
    assert np.all(alone["info"] == 0)
    for k in KEYS:
        assert np.array_equal(out[k][good], alone[k]), k
    for q in good:
        _feasible(out, lo[q], hi[q], q)
        ref = R.bvls(A[q], b[q], lo[q], hi[q])
        assert ref["info"] == 0 and np.array_equal(out["state"][q], ref["state"]), q
        got = R.measures(A[q], b[q], out["X"][q], out["W"][q], out["resid"][q], out["state"][q])
        rm = R.measures(A[q], b[q], ref["x"], ref["w"], ref["resid"], ref["state"])
        for k, name in enumerate(R.NAMES):
            _within(f"bvls special {m}x{n} member {q} {name}", (m, n, "special", name), got[k], rm[k], c["cap"])
    # the fixed variable: state -1, on its value, never freed
    assert out["state"][3][jf] == -1 and out["X"][3][jf] == 0.125
    # all unbounded: one elimination, all free, and the solution of qr_gels_batched_dev on the same member by the rule
    assert out["iter"][1] == 1 and np.all(out["state"][1] == 0)
    dA1 = torch.from_numpy(np.ascontiguousarray(A[1].T)).cuda()
    dB1 = torch.from_numpy(b[1].copy()).cuda()
    tau = torch.zeros(n, dtype=torch.float64, device="cuda")
    ginfo = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan.gels_batched(dA1, m, n, m, m * n, tau, n, dB1, 1, m, m, ginfo, 1)
    plan.sync()
    xg = dB1.cpu().numpy()[:n]
    free = np.zeros(n, dtype=int)
    sg = R.measures(A[1], b[1], xg, None, None, free)[0]
    so = R.measures(A[1], b[1], out["X"][1], None, None, free)[0]
    print(f"UNBOUNDED bvls {m}x{n}: bitwise qr_gels_batched_dev's x: {np.array_equal(xg, out['X'][1])}; max |dx| {np.max(np.abs(xg - out['X'][1])):.2e}")
    _within(f"bvls unbounded {m}x{n} stationarity against qr_gels_batched_dev", (m, n, "unbounded"), so, sg, c["cap"])
    # the host twin and the Python wrapper: the same members, zeros where nothing was computed; the wrapper does not raise
    Xw, ww, sw, rw, iw, fw = qr.lstsq_bounded_batched(A, b, lo, hi)
    assert np.array_equal(fw, want)
    assert np.array_equal(Xw[good], alone["X"]) and np.array_equal(ww[good], alone["W"]) and np.array_equal(sw[good], alone["state"])
    assert np.array_equal(rw[good], alone["resid"]) and np.array_equal(iw[good], alone["iter"])
    for q in bad:
        assert np.all(Xw[q] == 0.0) and np.all(ww[q] == 0.0) and np.all(sw[q] == 0) and rw[q] == 0.0 and iw[q] == 0
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    X = np.full((BATCH, n), 3.0)
    info = np.full(BATCH, ISENT, dtype=np.intc)
    At = np.ascontiguousarray(A.transpose(0, 2, 1))
    rc = qr.lib.qr_lstsq_bounded_batched(At.ctypes.data_as(dp), m, n, np.ascontiguousarray(b).ctypes.data_as(dp),
                                         np.ascontiguousarray(lo).ctypes.data_as(dp), np.ascontiguousarray(hi).ctypes.data_as(dp), 0, BATCH,
                                         X.ctypes.data_as(dp), None, None, None, None, info.ctypes.data_as(ip))
    assert rc == qr.QR_E_SINGULAR and np.array_equal(info, want) and np.array_equal(X[good], alone["X"])


@pytest.mark.parametrize("m,n", SPECIAL)
def test_nnls_through_a_null_upper_bound(plan, qr, m, n):
    c = R.case(m, n, salt=2)
    A, b = c["A"], c["b"]
    zero = np.zeros((BATCH, n))
    out = _solve(plan, A, b, zero, None)
    assert np.all(out["info"] == 0)
    assert _same(out, _solve(plan, A, b, zero, np.full((BATCH, n), INF))), "a NULL dhi is +inf"
    assert _same(out, _solve(plan, A, b, np.zeros(n), None, shared=True))
    for q in range(BATCH):
        _feasible(out, zero[q], np.full(n, INF), q)
        ref = R.bvls(A[q], b[q], zero[q], None)
        assert ref["info"] == 0 and np.array_equal(out["state"][q], ref["state"]), q
        assert np.all(out["W"][q][out["state"][q] == -1] <= 0)
        got = R.measures(A[q], b[q], out["X"][q], out["W"][q], out["resid"][q], out["state"][q])
        rm = R.measures(A[q], b[q], ref["x"], ref["w"], ref["resid"], ref["state"])
        for k, name in enumerate(R.NAMES):
            _within(f"nnls {m}x{n} member {q} {name}", (m, n, "nnls", name), got[k], rm[k], c["cap"])
    Xw, ww, sw, rw, iw, fw = qr.nnls_batched(A, b)
    assert np.array_equal(Xw, out["X"]) and np.array_equal(sw, out["state"]) and np.array_equal(iw, out["iter"]) and np.all(fw == 0)
    # all unbounded through two NULL pointers
    free = _solve(plan, A, b, None, None)
    assert np.all(free["info"] == 0) and np.all(free["iter"] == 1) and np.all(free["state"] == 0)
    assert _same(free, _solve(plan, A, b, np.full((BATCH, n), -INF), np.full((BATCH, n), INF)))


@pytest.mark.parametrize("m,n", SPECIAL)
def test_maxit_one_returns_a_feasible_iterate(plan, m, n):
    c = R.case(m, n)
    out = _case_solve(plan, c, maxit=1)
    full = _case_solve(plan, c)
    hit = 0
    for q in range(BATCH):
        if full["iter"][q] > 1:
            hit += 1
            assert out["info"][q] == n + 1 and out["iter"][q] == 1
        else:
            assert out["info"][q] == 0 and all(np.array_equal(out[k][q], full[k][q]) for k in KEYS)
        _feasible(out, c["lo"][q], c["hi"][q], q)
        got = R.measures(c["A"][q], c["b"][q], out["X"][q], out["W"][q], out["resid"][q], out["state"][q])
        assert got[1] <= c["cap"] and got[2] <= c["cap"], (q, got)          # w and resid belong to the iterate returned
    assert hit >= BATCH // 2
