"""-m gpu: batched inequality-constrained least squares (mi355x_qr.h section 8l), member by member.

Shapes, the planted inputs, the restatement of the method and the measures: tests/batched_lsei_ref.py.  The shapes cover the wave route
(its smallest member, each register width, both of its edges m == 64 and n + 1 == 32, mg == 64) and the workgroup route (the first shapes
past each edge, m == n at full width, qr_lsei_batched_max_rows(63, 64) rows).  Every buffer has an odd stride larger than packed (A and G
an odd leading dimension too), a base one element off, and is sentinel-filled outside its blocks; nothing outside the blocks may change
and the inputs may not change at all.  Batches are 9, 5 and 1.

Asserted on every member of the planted inputs: info == 0, the planted state exactly, mu > 0 on the inequalities of the set and exactly 0
off it, the count equal to the float64 restatement's, and the four measures (feasibility, kkt, resid, s) within the rule of
test_gpu_range_edges.py: each <= min(max(4 x the same measure of the float64 restatement on the same input, eps), cap).  A case that
exceeds 4 x on the GPU is listed in MEASURED at its measured ratio and bounded at twice that; the cap holds for it all the same (one
case: an equality row at 8 x 7).  The ratios and the counts are printed (-s) and tabulated in DESIGN.md section 7s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batched_lsei_ref as R

pytestmark = pytest.mark.gpu

EPS = R.EPS
SENTINEL = -7.25e33
ISENT = 77
BATCH = R.BATCH

# (m, n, mg, neq, measure) -> the ratio to the float64 restatement (floored at eps / 4, as in the rule) measured on an MI355X where it
# exceeds 4; the bound of such a case is twice the ratio, and never above the cap
MEASURED = {(8, 7, 3, 1, "feasibility"): 7.52}       # member 8: 1.9 eps on an equality row against 0.15 eps; the cap is 15 eps

# the shapes of the exact-property and special-member tests: both routes, each register width of the wave route, m == n at full width
EXACT = [(3, 2, 5, 0), (8, 7, 3, 1), (16, 15, 15, 0), (64, 31, 40, 0), (65, 31, 10, 0), (40, 32, 33, 3), (63, 63, 64, 0)]
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


def _solve(plan, A, b, G, h, neq, maxit=0, rcond=0.0, shared=False, want=("mu", "s", "state", "resid", "iter")):
    """one qr_lsei_batched_dev call on members A (batch, m, n), b (batch, m), G (batch, mg, n), h (batch, mg); with shared=True G is
    (mg, n) and h (mg,), passed with stride 0"""
    bt, m, n = A.shape
    mg = G.shape[-2]
    dA, dB = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None])
    nb = 1 if shared else bt
    dG = Strided(mg, n, nb, np.reshape(G, (nb, mg, n)))
    dH = Strided(mg, 1, nb, np.reshape(h, (nb, mg, 1)))
    dX, dMU, dS, dst = Strided(n, 1, bt), Strided(mg, 1, bt), Strided(mg, 1, bt), Strided(mg, 1, bt, dtype=np.int32)
    dres = torch.full((bt + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    dit = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    dinfo = torch.full((bt + 2,), ISENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kw = dict(maxit=maxit, rcond=rcond)
    if "mu" in want:
        kw.update(dMU=dMU.ptr, strideMU=dMU.stride)
    if "s" in want:
        kw.update(dS=dS.ptr, strideS=dS.stride)
    if "state" in want:
        kw.update(dstate=dst.ptr, stridestate=dst.stride)
    if "resid" in want:
        kw.update(dresid=dres[1:])
    if "iter" in want:
        kw.update(diter=dit[1:])
    plan.lsei_batched(dA.ptr, m, n, dA.ld, dA.stride, dB.ptr, dB.stride, dG.ptr, mg, neq, dG.ld, 0 if shared else dG.stride, dH.ptr,
                      0 if shared else dH.stride, dX.ptr, dX.stride, dinfo[1:], bt, **kw)
    plan.sync()
    for buf in (dA, dB, dG, dH):
        assert buf.unchanged(), "the inputs and their padding are untouched"
    for name, buf in (("mu", dMU), ("s", dS), ("state", dst)):
        if name not in want:
            assert buf.unchanged(), name
    res, it, info = dres.cpu().numpy(), dit.cpu().numpy(), dinfo.cpu().numpy()
    assert res[0] == SENTINEL and res[-1] == SENTINEL and it[0] == ISENT and it[-1] == ISENT and info[0] == ISENT and info[-1] == ISENT
    if "resid" not in want:
        assert np.all(res == SENTINEL)
    if "iter" not in want:
        assert np.all(it == ISENT)
    return dict(X=dX.get()[:, :, 0], MU=dMU.get()[:, :, 0], S=dS.get()[:, :, 0], state=dst.get()[:, :, 0], resid=res[1:-1], iter=it[1:-1],
                info=info[1:-1])


def _case_solve(plan, c, neq, idx=None, **kw):
    idx = list(range(len(c["A"]))) if idx is None else idx
    return _solve(plan, c["A"][idx], c["b"][idx], c["G"][idx], c["h"][idx], neq, **kw)


KEYS = ("X", "MU", "S", "state", "resid", "iter", "info")


def _same(a, b, keys=KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys)


def _within(tag, key, got, ref, cap):
    factor = 2.0 * MEASURED[key] if key in MEASURED else 4.0
    bound = min(factor * max(ref, EPS / 4), cap)             # (factor 4: min(max(4 ref, eps), cap), the rule)
    print(f"RATIO {tag}: {got:.3e} is {got / max(ref, EPS / 4):.2f} x the float64 reference {ref:.3e}; bound {bound:.3e} (cap {cap:.3e})")
    assert np.isfinite(got) and got <= bound, (tag, got, ref, bound)


def _multipliers(out, neq, q):
    mu, st = out["MU"][q], out["state"][q]
    assert np.all(np.isin(st, (0, 1))) and np.all(st[:neq] == 1)
    assert np.all(mu[neq:][st[neq:] == 1] > 0), (q, "mu > 0 on the inequalities of the set")
    assert np.all(mu[st == 0] == 0.0), (q, "mu is exactly 0 off the set")


def _measured(tag, shape, member, out, q, ref, caps):
    A, b, G, h = member
    got = R.measures(A, b, G, h, out["X"][q], out["MU"][q], out["S"][q], out["resid"][q], out["state"][q])
    fails = []
    for k, name in enumerate(R.NAMES):
        try:
            _within(f"{tag} member {q} {name}", shape + (name,), got[k], ref[k], caps[k])
        except AssertionError as e:
            fails.append(e.args[0])
    return got, fails


# ------------------------------------------------------------------------------------------------
# the planted inputs, every shape
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,mg,neq", R.SHAPES)
def test_planted_members_state_multipliers_count_and_accuracy(plan, qr, m, n, mg, neq):
    assert bool(qr.lib.qrd_le_wave_route(m, n)) == ((m, n, mg, neq) in R.WAVE_SHAPES)
    assert m <= qr.lsei_batched_max_rows(n, mg)
    c = R.case(m, n, mg, neq)
    out = _case_solve(plan, c, neq)
    assert np.all(out["info"] == 0), out["info"]
    worst = [0.0] * 4
    fails = []
    for q in range(BATCH):
        assert np.array_equal(out["state"][q], c["state"][q]), (q, "the planted state")
        _multipliers(out, neq, q)
        assert out["iter"][q] == c["out64"][q]["iter"], (q, "the count of the float64 restatement", out["iter"][q], c["out64"][q]["iter"])
        got, f = _measured(f"lsei {m}x{n} mg {mg} neq {neq}", (m, n, mg, neq), (c["A"][q], c["b"][q], c["G"][q], c["h"][q]), out, q,
                           c["ref"][q], c["caps"])
        fails += f
        for k in range(4):
            worst[k] = max(worst[k], got[k] / max(c["ref"][q][k], EPS / 4))
    print(f"WORST lsei {m}x{n} mg {mg} neq {neq}: " + ", ".join(f"{name} {w:.2f} x" for name, w in zip(R.NAMES, worst)) +
          f" the float64 reference; candidates mean {np.mean(out['iter']):.1f} max {np.max(out['iter'])} of {3 * mg + 1}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------
# exact properties, bitwise
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,mg,neq", EXACT)
def test_repeatable_and_independent_of_batch_index_and_optional_outputs(plan, m, n, mg, neq):
    c = R.case(m, n, mg, neq)
    full = _case_solve(plan, c, neq)
    assert _same(full, _case_solve(plan, c, neq)), "repeated calls are equal"
    perm = [7, 2, 8, 0, 4]
    sub = _case_solve(plan, c, neq, perm)                     # batch 5: a workgroup of the wave route that is not full
    for k in KEYS:
        assert np.array_equal(sub[k], full[k][perm]), k
    one = _case_solve(plan, c, neq, [3])                      # batch 1
    for k in KEYS:
        assert np.array_equal(one[k], full[k][[3]]), k
    bare = _case_solve(plan, c, neq, want=())                 # NULL optional outputs: their buffers stay untouched (_solve)
    assert np.array_equal(bare["X"], full["X"]) and np.array_equal(bare["info"], full["info"])
    some = _case_solve(plan, c, neq, perm, want=("mu", "iter"))
    assert np.array_equal(some["X"], full["X"][perm]) and np.array_equal(some["MU"], full["MU"][perm])
    assert np.array_equal(some["iter"], full["iter"][perm])
    # one G and h for all members (stride 0) against per-member copies of them
    G0, h0 = c["G"][4].copy(), c["h"][4].copy()
    tiled = _solve(plan, c["A"], c["b"], np.tile(G0, (BATCH, 1, 1)), np.tile(h0, (BATCH, 1)), neq)
    assert _same(tiled, _solve(plan, c["A"], c["b"], G0, h0, neq, shared=True)), "shared G and h equal per-member copies"


@pytest.mark.parametrize("m,n,mg,neq", EXACT)
def test_scaling_by_powers_of_two_is_exact(plan, m, n, mg, neq):
    c = R.case(m, n, mg, neq)
    idx = [0, 1, 2, 3, 4]                                     # batch 5: plain and graded members
    A, b, G, h = (c[k][idx] for k in ("A", "b", "G", "h"))
    base = _solve(plan, A, b, G, h, neq)
    assert np.all(base["info"] == 0)
    for ea, ec in ((20, 0), (-20, 0), (0, 9), (0, -11), (6, -7)):
        sa, sc = 2.0 ** ea, 2.0 ** ec
        out = _solve(plan, sa * A, sa * b, sc * G, sc * h, neq)
        assert _same(out, base, ("X", "state", "iter", "info")), (ea, ec)
        assert np.array_equal(out["MU"], (sa * sa / sc) * base["MU"]), (ea, ec)
        assert np.array_equal(out["resid"], sa * base["resid"]) and np.array_equal(out["S"], sc * base["S"]), (ea, ec)


@pytest.mark.parametrize("m,n,p", [(8, 7, 3), (16, 15, 15), (64, 31, 7), (65, 31, 7), (40, 32, 31), (130, 63, 20), (30, 63, 40)])
def test_all_equalities_is_gglse_bit_for_bit(plan, m, n, p):
    rng = np.random.default_rng(1000 * m + 10 * n + p)
    bt = 5
    A, b = rng.standard_normal((bt, m, n)), rng.standard_normal((bt, m))
    G, h = rng.standard_normal((bt, p, n)), rng.standard_normal((bt, p))
    out = _solve(plan, A, b, G, h, p)
    assert np.all(out["info"] == 0) and np.all(out["iter"] == 1) and np.all(out["state"] == 1)
    dA, dB, dC, dD = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None]), Strided(p, n, bt, G), Strided(p, 1, bt, h[:, :, None])
    dX, dL = Strided(n, 1, bt), Strided(p, 1, bt)
    dres = torch.zeros(bt, dtype=torch.float64, device="cuda")
    ginfo = torch.full((bt,), ISENT, dtype=torch.int32, device="cuda")
    plan.gglse_batched(dA.ptr, m, n, dA.ld, dA.stride, dC.ptr, p, dC.ld, dC.stride, dB.ptr, dB.ld, dB.stride, dD.ptr, dD.ld, dD.stride, 1,
                       dX.ptr, dX.ld, dX.stride, ginfo, bt, dL=dL.ptr, ldl=dL.ld, strideL=dL.stride, dresid=dres, strideres=1)
    plan.sync()
    assert np.all(ginfo.cpu().numpy() == 0)
    assert np.array_equal(out["X"], dX.get()[:, :, 0]), "x is qr_gglse_batched_dev's bit for bit"
    assert np.array_equal(out["MU"], -dL.get()[:, :, 0]), "mu is minus its multipliers"


@pytest.mark.parametrize("m,n,mg", [(8, 7, 3), (16, 15, 15), (64, 31, 40), (65, 31, 10), (100, 33, 64), (63, 63, 64)])
def test_all_slack_is_gels_bit_for_bit(plan, m, n, mg):
    rng = np.random.default_rng(1000 * m + 10 * n + mg + 5)
    bt = 5
    A, b, G = rng.standard_normal((bt, m, n)), rng.standard_normal((bt, m)), rng.standard_normal((bt, mg, n))
    x0 = np.stack([np.linalg.lstsq(A[q], b[q], rcond=None)[0] for q in range(bt)])
    h = np.einsum("qij,qj->qi", G, x0) - rng.uniform(0.5, 1.5, (bt, mg))
    out = _solve(plan, A, b, G, h, 0)
    assert np.all(out["info"] == 0) and np.all(out["iter"] == 1) and np.all(out["state"] == 0) and np.all(out["MU"] == 0.0)
    assert np.all(out["S"] > 0)
    dA = torch.from_numpy(np.ascontiguousarray(A.transpose(0, 2, 1))).cuda()
    dB = torch.from_numpy(b.copy()).cuda()
    tau = torch.zeros(bt * n, dtype=torch.float64, device="cuda")
    ginfo = torch.zeros(bt, dtype=torch.int32, device="cuda")
    plan.gels_batched(dA, m, n, m, m * n, tau, n, dB, 1, m, m, ginfo, bt)
    plan.sync()
    assert np.all(ginfo.cpu().numpy() == 0)
    assert np.array_equal(out["X"], dB.cpu().numpy()[:, :n]), "x is qr_gels_batched_dev's bit for bit"


# ------------------------------------------------------------------------------------------------
# special members beside unaffected neighbours
# ------------------------------------------------------------------------------------------------
def _embed(n, mg, G2, h2):
    """the rows (G2, h2) on the first two unknowns, padded to mg rows by rows 0 x >= -1 and to n unknowns by zero columns"""
    G, h = np.zeros((mg, n)), -np.ones(mg)
    G[:len(h2), :G2.shape[1]] = G2
    h[:len(h2)] = h2
    return G, h


@pytest.mark.parametrize("m,n", SPECIAL)
def test_special_members_and_their_neighbours(plan, qr, m, n):
    mg = 6
    c = R.case(m, n, mg, 0, salt=1)
    A, b, G, h = (c[k].copy() for k in ("A", "b", "G", "h"))
    # members 1, 2, 5: A = [I ; 0], b = the last unit vector, orthogonal to range A (x is the point of the set nearest the origin)
    for q in (1, 2, 5):
        A[q], b[q] = np.eye(m, n), np.eye(m)[m - 1]
    G[1], h[1] = _embed(n, mg, *R.DEPENDENT_FEASIBLE)          # dependent but feasible: info 0 after 3 candidates
    G[2], h[2] = _embed(n, mg, *R.INFEASIBLE)                  # infeasible: -2
    G[5], h[5] = _embed(n, mg, np.array([[2.0, 0.0], [1.0, 0.0]]), np.array([1.0, 1.0]))     # a dependent row that is violated: 4 passes
    G[6][3], h[6][3] = 0.0, -0.5                               # a zero row with h <= 0: never violated
    G[8][2], h[8][2] = 0.0, 0.25                               # a zero row with h > 0: -2
    want = np.zeros(BATCH, dtype=np.int32)
    want[[2, 8]] = -2
    bad = [2, 8]
    good = [q for q in range(BATCH) if q not in bad]
    out = _solve(plan, A, b, G, h, 0)
    assert np.array_equal(out["info"], want), out["info"]
    for q in bad:                                              # nothing but info is written
        assert np.all(out["X"][q] == SENTINEL) and np.all(out["MU"][q] == SENTINEL) and np.all(out["S"][q] == SENTINEL)
        assert np.all(out["state"][q] == ISENT) and out["resid"][q] == SENTINEL and out["iter"][q] == ISENT
    alone = _solve(plan, A[good], b[good], G[good], h[good], 0)
    assert np.all(alone["info"] == 0)
    for k in KEYS:
        assert np.array_equal(out[k][good], alone[k]), k
    for q in good:
        _multipliers(out, 0, q)
        ref = R.lsei(A[q], b[q], G[q], h[q], 0)
        assert ref["info"] == 0 and np.array_equal(out["state"][q], ref["state"]) and out["iter"][q] == ref["iter"], q
        rm = R.measures(A[q], b[q], G[q], h[q], ref["x"], ref["mu"], ref["s"], ref["resid"], ref["state"])
        _, fails = _measured(f"lsei special {m}x{n}", (m, n, "special"), (A[q], b[q], G[q], h[q]), out, q, rm, c["caps"])
        assert not fails, fails
    x1 = np.zeros(n)
    x1[:2] = 1.0, 0.5
    assert np.array_equal(out["X"][1], x1) and out["iter"][1] == 3 and np.array_equal(out["state"][1], [1, 0, 1, 0, 0, 0])
    x5 = np.zeros(n)
    x5[0] = 1.0
    assert np.array_equal(out["X"][5], x5) and out["iter"][5] == 4 and np.array_equal(out["state"][5], [0, 1, 0, 0, 0, 0])
    assert out["state"][6][3] == 0 and out["S"][6][3] == 0.5
    # the host twin and the Python wrapper: the same members, zeros where nothing was computed; the wrapper does not raise
    Xw, mw, sw, stw, rw, iw, fw = qr.lstsq_inequality_batched(A, b, G, h)
    assert np.array_equal(fw, want)
    assert np.array_equal(Xw[good], alone["X"]) and np.array_equal(mw[good], alone["MU"]) and np.array_equal(sw[good], alone["S"])
    assert np.array_equal(stw[good], alone["state"]) and np.array_equal(rw[good], alone["resid"]) and np.array_equal(iw[good], alone["iter"])
    for q in bad:
        assert np.all(Xw[q] == 0.0) and np.all(mw[q] == 0.0) and np.all(sw[q] == 0.0) and np.all(stw[q] == 0) and rw[q] == 0.0 and iw[q] == 0
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    X = np.full((BATCH, n), 3.0)
    info = np.full(BATCH, ISENT, dtype=np.intc)
    At, Gt = np.ascontiguousarray(A.transpose(0, 2, 1)), np.ascontiguousarray(G.transpose(0, 2, 1))
    rc = qr.lib.qr_lstsq_inequality_batched(At.ctypes.data_as(dp), m, n, np.ascontiguousarray(b).ctypes.data_as(dp), Gt.ctypes.data_as(dp), mg,
                                            0, np.ascontiguousarray(h).ctypes.data_as(dp), 0, 0.0, BATCH, X.ctypes.data_as(dp), None, None,
                                            None, None, None, info.ctypes.data_as(ip))
    assert rc == qr.QR_E_SINGULAR and np.array_equal(info, want) and np.array_equal(X[good], alone["X"])


@pytest.mark.parametrize("m,n,mg,neq", [(16, 7, 20, 2), (64, 31, 40, 0), (40, 32, 33, 3), (130, 63, 64, 8)])
def test_maxit_two_returns_the_last_accepted_pair(plan, m, n, mg, neq):
    c = R.case(m, n, mg, neq)
    out = _case_solve(plan, c, neq, maxit=2)
    full = _case_solve(plan, c, neq)
    hit = 0
    for q in range(BATCH):
        ref = R.lsei(c["A"][q], c["b"][q], c["G"][q], c["h"][q], neq, maxit=2)
        assert out["info"][q] == ref["info"] and out["iter"][q] == ref["iter"] and np.array_equal(out["state"][q], ref["state"]), q
        if full["iter"][q] > 2:
            hit += 1
            assert out["info"][q] == n + 1 and out["iter"][q] == 2
            assert np.min(out["S"][q][neq:]) < 0, (q, "s shows what the pair still violates")
        else:
            assert out["info"][q] == 0 and all(np.array_equal(out[k][q], full[k][q]) for k in KEYS)
        _multipliers(out, neq, q)
        got = R.measures(c["A"][q], c["b"][q], c["G"][q], c["h"][q], out["X"][q], out["MU"][q], out["S"][q], out["resid"][q],
                         np.zeros(mg, dtype=int))
        assert got[1] <= c["caps"][1] and got[2] <= c["caps"][2] and got[3] <= c["caps"][3], (q, got)     # the pair is a stationary one
    assert hit >= BATCH // 2
