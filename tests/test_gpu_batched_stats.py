"""-m gpu: batched covariance, standard errors and leverages (mi355x_qr.h section 8k), member by member.

Shapes, inputs, the restatement and the measures: tests/batched_stats_ref.py.  The fused shapes cover the wave route (its smallest
member, each register width, both edges m == 64 and n + 1 == 32) and the workgroup route (the first shapes past each edge, 256 x 63,
512 x 31); the from-factor calls run at n = 1, 2, 7, 31, 32 (one wave per member) and 33, 63, 64 (one workgroup).  The principal buffers
have an odd stride larger than packed (A and C an odd leading dimension too), a base one element off, and are sentinel-filled outside
their blocks; nothing outside the blocks may change and the inputs may not change at all.  Batches are 9, 5 and 1.

Accuracy, on every member, against the longdouble restatement, kappa the 2-norm condition of diag(sqrt(p)) A: the measures C, se and h
each <= 50 kappa eps (the hard cap), and each also <= 4 max(the same measure of the float64 restatement, eps / 4) unless the case is
listed in MEASURED with its measured ratio, which is admitted only below a quarter of the cap.  x: batched_irls_ref's scaled error <=
50 kappa' eps, the bound test_gpu_batched_irls.py applies to QR_LOSS_LS.  e and sigma2: within (m + n) eps of the scales of
batched_stats_ref.residual_scales, whose docstring derives them.

The scaled covariance is measured against sigma2 C_ref with the sigma2 the call itself returned: sigma2 is a sum of squares of
residuals that are small against b, so its own relative error is about eps ||b|| / ||e||, not kappa eps (the float64 restatement shows
68 kappa eps on 5 x 3 against sigma2_ref C_ref); sigma2 has its own bound above, and C_scaled == sigma2 * C_unscaled is asserted bitwise.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import batched_irls_ref as IR
import batched_stats_ref as S
import hp_ref as H

pytestmark = pytest.mark.gpu

EPS = S.EPS
SENTINEL = -7.25e33
ISENT = 77
BATCH = S.BATCH
NAN = float("nan")

# (m, n, weighted, measure) -> the ratio to the float64 restatement (floored at eps / 4) measured on an MI355X where it exceeds 4
# (DESIGN.md section 7r); such a case must stay below a quarter of the hard cap and within twice the listed ratio.  All six are far
# inside the cap: 1.26 kappa eps for 2 x 1, 0.48 kappa eps for 16 x 8, below 0.01 kappa eps for the others (graded members, kappa ~ 1e4)
MEASURED = {(2, 1, False, "C"): 5.04, (5, 3, False, "h"): 4.69, (5, 3, True, "C"): 6.15, (5, 3, True, "h"): 5.02, (16, 8, True, "se"): 5.16,
            (100, 33, False, "C"): 4.21}

EXACT = [(5, 3), (16, 8), (64, 31), (64, 32), (65, 15), (100, 33)]


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


def _flat(n, fill, dtype):
    return torch.full((n + 2,), fill, dtype=dtype, device="cuda")


def _ends(v, s):
    v = v.cpu().numpy()
    assert v[0] == s and v[-1] == s
    return v[1:-1]


ALL = ("E", "H", "sigma2", "dof", "C", "se")


def _fit(plan, qr, A, b, p=None, shared=False, scaled=True, want=ALL):
    """one qr_gels_stats_batched_dev call on members A (batch, m, n), b (batch, m); p: None (a NULL pointer), (batch, m), or with
    shared=True (m,) passed with stride 0.  Outputs not in `want` are passed as NULL and must stay at the sentinel"""
    bt, m, n = A.shape
    dA, dB = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None])
    nb = 1 if shared else bt
    dP = None if p is None else Strided(m, 1, nb, np.reshape(p, (nb, m, 1)))
    dX, dE, dH, dC, dse = Strided(n, 1, bt), Strided(m, 1, bt), Strided(m, 1, bt), Strided(n, n, bt), Strided(n, 1, bt)
    dsig, ddof, dinfo = _flat(bt, SENTINEL, torch.float64), _flat(bt, ISENT, torch.int32), _flat(bt, ISENT, torch.int32)
    torch.cuda.synchronize()
    kw = dict(scaled=qr.QR_COV_SCALED if scaled else qr.QR_COV_UNSCALED, strideprior=0 if shared else dE.stride)
    if dP is not None:
        kw.update(dprior=dP.ptr)
    if "E" in want:
        kw.update(dE=dE.ptr, strideE=dE.stride)
    if "H" in want:
        kw.update(dH=dH.ptr, strideH=dH.stride)
    if "sigma2" in want:
        kw.update(dsigma2=dsig[1:])
    if "dof" in want:
        kw.update(ddof=ddof[1:])
    if "C" in want:
        kw.update(dC=dC.ptr, ldc=dC.ld, strideC=dC.stride)
    if "se" in want:
        kw.update(dse=dse.ptr, stridese=dse.stride)
    plan.gels_stats_batched(dA.ptr, m, n, dA.ld, dA.stride, dB.ptr, dB.stride, dX.ptr, dX.stride, dinfo[1:], bt, **kw)
    plan.sync()
    for buf in (dA, dB, dP):
        assert buf is None or buf.unchanged(), "the inputs and their padding are untouched"
    for name, buf in (("E", dE), ("H", dH), ("C", dC), ("se", dse)):
        if name not in want:
            assert buf.unchanged()
    sig, dof, info = _ends(dsig, SENTINEL), _ends(ddof, ISENT), _ends(dinfo, ISENT)
    if "sigma2" not in want:
        assert np.all(sig == SENTINEL)
    if "dof" not in want:
        assert np.all(dof == ISENT)
    return dict(x=dX.get()[:, :, 0], e=dE.get()[:, :, 0], h=dH.get()[:, :, 0], C=dC.get(), se=dse.get()[:, :, 0], sigma2=sig, dof=dof, info=info)


def _ints(v):
    return None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).cuda()


def _covar(plan, R, jpvt=None, rank=None, mult=None, want=("C", "se"), ld=None, stride=None):
    """one qr_covar_batched_dev call on the n x n blocks R (batch, n, n): a Strided buffer (whose lower triangles hold whatever R holds),
    or with ld / stride given a device tensor holding in-place factors"""
    if ld is None:
        bt, n, _ = R.shape
        dR = Strided(n, n, bt, R)
        rptr, ld, stride = dR.ptr, dR.ld, dR.stride
    else:
        rptr, bt, n = R
        dR = None
    dC, dse = Strided(n, n, bt), Strided(n, 1, bt)
    dinfo = _flat(bt, ISENT, torch.int32)
    dj, dr = _ints(jpvt), _ints(rank)
    dm = None if mult is None else torch.from_numpy(np.ascontiguousarray(mult, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    kw = {}
    if "C" in want:
        kw.update(dC=dC.ptr, ldc=dC.ld, strideC=dC.stride)
    if "se" in want:
        kw.update(dse=dse.ptr, stridese=dse.stride)
    plan.covar_batched(rptr, n, ld, stride, dinfo[1:], bt, djpvt=dj, stridejpvt=n if dj is not None else 0, drank=dr, dmult=dm, **kw)
    plan.sync()
    assert dR is None or dR.unchanged()
    for name, buf in (("C", dC), ("se", dse)):
        if name not in want:
            assert buf.unchanged()
    return dict(C=dC.get(), se=dse.get()[:, :, 0], info=_ends(dinfo, ISENT))


def _lev(plan, R, rows, p=None, shared=False, jpvt=None, rank=None, ld=None, stride=None):
    """one qr_leverage_batched_dev call: R as in _covar, rows (batch, mrows, n)"""
    bt, mrows, n = rows.shape
    if ld is None:
        dR = Strided(n, n, bt, R)
        rptr, ld, stride = dR.ptr, dR.ld, dR.stride
    else:
        rptr, dR = R[0], None
    dA = Strided(mrows, n, bt, rows)
    nb = 1 if shared else bt
    dP = None if p is None else Strided(mrows, 1, nb, np.reshape(p, (nb, mrows, 1)))
    dH = Strided(mrows, 1, bt)
    dinfo = _flat(bt, ISENT, torch.int32)
    dj, dr = _ints(jpvt), _ints(rank)
    torch.cuda.synchronize()
    plan.leverage_batched(rptr, n, ld, stride, dA.ptr, mrows, dA.ld, dA.stride, dH.ptr, dH.stride, dinfo[1:], bt,
                          dprior=None if dP is None else dP.ptr, strideprior=0 if shared else dH.stride, djpvt=dj,
                          stridejpvt=n if dj is not None else 0, drank=dr)
    plan.sync()
    for buf in (dR, dA, dP):
        assert buf is None or buf.unchanged()
    return dict(h=dH.get()[:, :, 0], info=_ends(dinfo, ISENT))


def _planted(m, n, weighted):
    """the case's members with NaN planted in the masked rows of A and b"""
    A, b, p = S.make_case(m, n, weighted)
    A, b = A.copy(), b.copy()
    if p is not None:
        for q in range(len(A)):
            A[q][p[q] == 0, :] = NAN
            b[q][p[q] == 0] = NAN
    return A, b, p


def _bound(name, m, n, weighted, ref_err, kap):
    """min(4 max(the float64 restatement's measure, eps / 4), cap), or for a MEASURED case twice its ratio below a quarter of the cap"""
    cap = S.CAP * kap * EPS
    floor = max(ref_err, EPS / 4)
    key = (m, n, weighted, name)
    if key in MEASURED:
        return min(2 * MEASURED[key] * floor, 0.25 * cap), cap, floor
    return min(4 * floor, cap), cap, floor


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("m,n", S.FIT_SHAPES, ids=[f"{m}x{n}" for m, n in S.FIT_SHAPES])
def test_fused_fit_accuracy_and_identities(plan, qr, m, n, weighted):
    A, b, p = _planted(m, n, weighted)
    A0, b0, _ = S.make_case(m, n, weighted)
    refs = S.reference_case(m, n, weighted)
    un = _fit(plan, qr, A, b, p, scaled=False)
    sc = _fit(plan, qr, A, b, p, scaled=True)
    assert np.all(un["info"] == 0)
    if m == n:
        assert np.all(sc["info"] == -3) and np.all(sc["x"] == SENTINEL) and np.all(sc["C"] == SENTINEL) and np.all(sc["e"] == SENTINEL)
        assert np.all(un["sigma2"] == np.inf) and np.all(un["dof"] == 0)
    else:
        assert np.all(sc["info"] == 0)
    failures = []
    for q, (ld, f64, kap) in enumerate(refs):
        pq = np.ones(m) if p is None else p[q]
        for out, scaled in ((un, False), (sc, True)):
            if scaled and m == n:
                continue
            o = {k: out[k][q] for k in ("x", "e", "h", "C", "se", "sigma2", "dof")}
            ref = S.scaled_reference(ld, o["sigma2"]) if scaled else ld
            r64 = S.errors(S.with_scale(f64) if scaled else f64, S.scaled_reference(ld, f64["sigma2"]) if scaled else ld)
            err = S.errors(o, ref)
            for name in S.NAMES:
                bound, cap, floor = _bound(name, m, n, weighted, r64[name], kap)
                print(f"{m}x{n} weighted={weighted} scaled={scaled} q={q} {name}: {err[name] / (kap * EPS):.3f} kappa eps, "
                      f"{err[name] / floor:.2f} x float64")
                assert err[name] <= cap, (q, scaled, name, err[name] / (kap * EPS))
                if err[name] > bound:
                    failures.append((q, scaled, name, err[name] / floor))
            # the identities on the device results
            assert np.array_equal(o["C"], o["C"].T)
            assert np.array_equal(o["se"], np.sqrt(np.diagonal(o["C"])))
            assert abs(o["h"].sum() - n) <= (m + n) * EPS * n
            assert o["h"].min() >= -EPS and o["h"].max() <= 1 + S.CAP * kap * EPS
            assert np.all(o["h"][pq == 0] == 0.0) and np.all(o["e"][pq == 0] == 0.0)
            assert o["dof"] == ld["dof"]
            # x, e, sigma2
            kx = IR.kappa(A0[q], pq)
            assert IR.scaled_error(A0[q], o["x"], ld["x"]) <= S.CAP * kx * EPS
            se_, ss_ = S.residual_scales(A0[q], b0[q], None if p is None else pq, ld)
            de = float(np.max(np.abs(np.asarray(H.arr(o["e"]) - ld["e"], dtype=np.float64))))
            assert de <= (m + n) * EPS * se_, (q, de / (EPS * se_))
            if ld["dof"] > 0:
                ds = abs(float(H.arr(np.float64(o["sigma2"])) - ld["sigma2"]))
                assert ds <= (m + n) * EPS * ss_, (q, ds / (EPS * ss_))
        if m > n:
            assert np.array_equal(sc["C"][q], un["sigma2"][q] * un["C"][q])       # one rounded product per entry
            for k in ("x", "e", "h", "sigma2", "dof"):
                assert np.array_equal(sc[k][q], un[k][q])
    assert not failures, f"above 4 x the float64 restatement and not in MEASURED: {failures}"


def _geqrf(plan, W):
    """the in-place factors of qr_geqrf_batched_dev for W (batch, m, n): (device tensor, lda, strideA, R as numpy)"""
    bt, m, n = W.shape
    dW = Strided(m, n, bt, W)
    dtau = torch.zeros(bt * n, dtype=torch.float64, device="cuda")
    plan.geqrf_batched(dW.ptr, m, n, dW.ld, dW.stride, dtau, n, bt)
    plan.sync()
    return dW


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("m,n", [(m, n) for m, n in S.FIT_SHAPES if m > n], ids=[f"{m}x{n}" for m, n in S.FIT_SHAPES if m > n])
def test_fused_results_equal_the_composed_calls_bitwise(plan, qr, m, n, weighted):
    A, b, p = S.make_case(m, n, weighted)
    bt = len(A)
    out = _fit(plan, qr, A, b, p, scaled=False)
    # x: qr_gels_batched_dev without weights, qr_gels_weighted_batched_dev with them.  qr_gels_batched_dev is one fused launch (the shared
    # column steps with b riding along) up to qr_batched_max_rows(n + 1) rows; above that (300 x 40 here) section 8 composes geqrf, ormqr
    # and trsm, and its ormqr adds Q^T b in another order, so its x is not the shared steps' x and no kernel can equal both: there x is
    # compared with qr_gels_weighted_batched_dev at NULL weights alone, which runs at every shape
    dX, dinfo = Strided(n, 1, bt), _flat(bt, ISENT, torch.int32)
    if p is None and m <= qr.lib.qr_batched_max_rows(n + 1):
        dA, dB = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None])
        dtau = torch.zeros(bt * n, dtype=torch.float64, device="cuda")
        plan.gels_batched(dA.ptr, m, n, dA.ld, dA.stride, dtau, n, dB.ptr, 1, dB.ld, dB.stride, dinfo[1:], bt)
        plan.sync()
        assert np.array_equal(dB.get()[:, :n, 0], out["x"])
    assert p is not None or m <= qr.lib.qr_batched_max_rows(n + 1) or (m, n) == (300, 40)
    dA, dB = Strided(m, n, bt, A), Strided(m, 1, bt, b[:, :, None])
    dP = None if p is None else Strided(m, 1, bt, p[:, :, None])
    plan.gels_weighted_batched(dA.ptr, m, n, dA.ld, dA.stride, dB.ptr, dB.stride, None if dP is None else dP.ptr, dB.stride, dX.ptr, dX.stride,
                               dinfo[1:], bt)
    plan.sync()
    assert np.array_equal(dX.get()[:, :, 0], out["x"])
    # C, se and h: from the factors qr_geqrf_batched_dev leaves for the sqrt(p)-scaled A, where both column counts take one route
    if bool(qr.lib.qrd_b_wave_route(m, n)) == bool(qr.lib.qrd_b_wave_route(m, n + 1)) and qr.lib.qrd_b_fits(m, n + 1):
        W = A if p is None else A * np.sqrt(p)[:, :, None]
        dW = _geqrf(plan, W)
        cov = _covar(plan, (dW.ptr, bt, n), ld=dW.ld, stride=dW.stride)
        assert np.all(cov["info"] == 0)
        assert np.array_equal(cov["C"], out["C"]) and np.array_equal(cov["se"], out["se"])
        lev = _lev(plan, (dW.ptr,), A, p, ld=dW.ld, stride=dW.stride)
        assert np.all(lev["info"] == 0) and np.array_equal(lev["h"], out["h"])
        sc = _fit(plan, qr, A, b, p, scaled=True)
        cs = _covar(plan, (dW.ptr, bt, n), mult=out["sigma2"], ld=dW.ld, stride=dW.stride)
        assert np.array_equal(cs["C"], sc["C"]) and np.array_equal(cs["se"], sc["se"])


def _triangles(n, bt, graded=True):
    """well-conditioned upper triangles with junk (NaN) below the diagonal, which is never read"""
    rng = np.random.default_rng(8115000 + n)
    M = rng.standard_normal((bt, n + 6, n))
    if graded and n > 1:
        M[1::3] *= np.logspace(0, 4, n)[None, None, :]
    R = np.stack([np.linalg.qr(M[q], mode="r") for q in range(bt)])
    junk = np.tril(np.full((n, n), NAN), -1)
    return M, np.triu(R) + junk[None]


@pytest.mark.parametrize("n", S.FACTOR_N)
def test_from_factor_calls_against_the_restatement(plan, n):
    bt = BATCH
    M, R = _triangles(n, bt)
    rng = np.random.default_rng(8116000 + n)
    mult = rng.uniform(0.5, 3.0, bt)
    rows = rng.standard_normal((bt, 70, n)) * (np.linalg.norm(M, axis=1) / np.sqrt(n + 6))[:, None, :]
    pr = rng.uniform(0.25, 4.0, (bt, 70))
    pr[:, ::7] = 0.0
    rows[:, ::7, :] = NAN
    cov = _covar(plan, R, mult=mult)
    lev = _lev(plan, R, rows, pr)
    assert np.all(cov["info"] == 0) and np.all(lev["info"] == 0)
    only_se = _covar(plan, R, mult=mult, want=("se",))
    only_c = _covar(plan, R, mult=mult, want=("C",))
    assert np.array_equal(only_se["se"], cov["se"]) and np.array_equal(only_c["C"], cov["C"])
    for q in range(bt):
        Rq = np.triu(R[q])
        kap = float(np.linalg.cond(Rq))
        Cl, sel = S.covar_from_r(Rq, mult=mult[q], dtype=H.LD)
        hl = S.leverage_from_r(Rq, rows[q], pr[q], dtype=H.LD)
        C64, se64 = S.covar_from_r(Rq, mult=mult[q])
        h64 = S.leverage_from_r(Rq, rows[q], pr[q])
        err = S.errors(dict(C=cov["C"][q], se=cov["se"][q], h=lev["h"][q]), dict(C=Cl, se=sel, h=hl))
        r64 = S.errors(dict(C=C64, se=se64, h=h64), dict(C=Cl, se=sel, h=hl))
        for name in S.NAMES:              # (h of new points is not bounded by 1; its cap is the absolute one all the same)
            e, r = err[name], r64[name]
            print(f"n={n} q={q} {name}: {e / (kap * EPS):.3f} kappa eps, {e / max(r, EPS / 4):.2f} x float64")
            assert e <= S.CAP * kap * EPS, (q, name, e / (kap * EPS))
            assert e <= 4 * max(r, EPS / 4), (q, name, e / max(r, EPS / 4))
        assert np.array_equal(cov["C"][q], cov["C"][q].T) and np.array_equal(cov["se"][q], np.sqrt(np.diagonal(cov["C"][q])))
        assert np.all(lev["h"][q][::7] == 0.0)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.mark.parametrize("n", [7, 33, 64])
def test_pivoted_and_rank_deficient_members(plan, qr, n):
    bt, m = 5, n + 5
    ranks = [0, max(1, n // 3), n - 1, n - 2, n]
    A = np.stack([S.rank_deficient_case(n, r, 1, salt=q)[0] if r < n else np.random.default_rng(8117000 + n).standard_normal((m, n))
                  for q, r in enumerate(ranks)])
    A[3][:, 0] = 0.0                          # a zero and a duplicated column
    A[3][:, 1] = A[3][:, 2]
    dA = Strided(m, n, bt, A)
    dj = torch.zeros(bt * n, dtype=torch.int32, device="cuda")
    dtau = torch.zeros(bt * n, dtype=torch.float64, device="cuda")
    drank = torch.zeros(bt, dtype=torch.int32, device="cuda")
    plan.geqp3_batched(dA.ptr, m, n, dA.ld, dA.stride, dj, n, dtau, n, bt)
    plan.rank_batched(dA.ptr, m, n, dA.ld, dA.stride, drank, bt)
    plan.sync()
    jp, rk = dj.cpu().numpy().reshape(bt, n), drank.cpu().numpy()
    F = dA.get()
    assert rk[0] == 0 and rk[1] == ranks[1] and rk[2] == n - 1 and rk[4] == n and rk[3] <= n - 2
    cov = _covar(plan, (dA.ptr, bt, n), jpvt=jp, rank=rk, ld=dA.ld, stride=dA.stride)
    lev = _lev(plan, (dA.ptr,), A, None, jpvt=jp, rank=rk, ld=dA.ld, stride=dA.stride)
    assert np.all(cov["info"] == 0) and np.all(lev["info"] == 0)
    for q in range(bt):
        r = int(rk[q])
        Rq = np.triu(F[q][:n, :n])
        drop = jp[q][r:]
        C = cov["C"][q]
        assert np.all(_bits(C[drop, :]) == 0) and np.all(_bits(C[:, drop]) == 0) and np.all(_bits(cov["se"][q][drop]) == 0)
        assert np.array_equal(C, C.T)
        assert abs(lev["h"][q].sum() - r) <= 1e-9 * max(r, 1)
        if r == 0:
            assert np.all(_bits(C) == 0) and np.all(_bits(lev["h"][q]) == 0)
            continue
        kap = float(np.linalg.cond(Rq[:r, :r]))
        Cl, sel = S.covar_from_r(Rq, jp[q], r, dtype=H.LD)
        hl = S.leverage_from_r(Rq, A[q], None, jp[q], r, dtype=H.LD)
        err = S.errors(dict(C=C, se=cov["se"][q], h=lev["h"][q]), dict(C=Cl, se=sel, h=hl))
        for name in S.NAMES:
            assert err[name] <= S.CAP * kap * EPS, (q, name, err[name] / (kap * EPS))


def test_accumulator_covariance_equals_covar_on_its_triangle(plan, qr):
    for n, rows in ((7, 20), (33, 40)):
        bt = 5
        rng = np.random.default_rng(8118000 + n)
        A, b = rng.standard_normal((bt, rows, n)), rng.standard_normal((bt, rows))
        acc = qr.LsAccumulatorBatched(plan, n, 1, bt)
        dA, dB = Strided(rows, n, bt, A), Strided(rows, 1, bt, b[:, :, None])
        acc.push(dA.ptr, rows, dA.ld, dA.stride, dB.ptr, dB.ld, dB.stride)
        dR, ldr, sR, _, _, _, drss, drows = acc.factor()
        for scaled in (False, True):
            dC, dse = Strided(n, n, bt), Strided(n, 1, bt)
            dsig, dinfo = _flat(bt, SENTINEL, torch.float64), _flat(bt, ISENT, torch.int32)
            acc.covar(dinfo[1:], scaled=int(scaled), rhs=0, dC=dC.ptr, ldc=dC.ld, strideC=dC.stride, dse=dse.ptr, stridese=dse.stride,
                      dsigma2=dsig[1:])
            plan.sync()
            sig = _ends(dsig, SENTINEL)
            assert np.all(_ends(dinfo, ISENT) == 0)
            cov = _covar(plan, (dR, bt, n), mult=sig if scaled else None, ld=ldr, stride=sR)
            assert np.array_equal(cov["C"], dC.get()) and np.array_equal(cov["se"], dse.get()[:, :, 0])
            for q in range(bt):
                _, res = H.lstsq(A[q], b[q])
                assert abs(sig[q] - float(res) ** 2 / (rows - n)) <= 1e-10 * sig[q]
        acc.close()
    # a member that holds fewer than n rows: i + 1; scaled with rows == n: -3
    n, bt = 5, 3
    rng = np.random.default_rng(8118999)
    acc = qr.LsAccumulatorBatched(plan, n, 1, bt)
    for rows, scaled, want in ((3, True, 4), (3, False, 4), (2, True, -3), (2, False, 0)):       # 3 rows, then 5 in all
        A, b = rng.standard_normal((bt, rows, n)), rng.standard_normal((bt, rows))
        dA, dB = Strided(rows, n, bt, A), Strided(rows, 1, bt, b[:, :, None])
        if scaled:
            acc.push(dA.ptr, rows, dA.ld, dA.stride, dB.ptr, dB.ld, dB.stride)
        dC, dsig, dinfo = Strided(n, n, bt), _flat(bt, SENTINEL, torch.float64), _flat(bt, ISENT, torch.int32)
        acc.covar(dinfo[1:], scaled=int(scaled), dC=dC.ptr, ldc=dC.ld, strideC=dC.stride, dsigma2=dsig[1:])
        plan.sync()
        assert np.all(_ends(dinfo, ISENT) == want), (rows, scaled, _ends(dinfo, ISENT))
        if want:
            assert dC.unchanged() and np.all(_ends(dsig, SENTINEL) == SENTINEL)
        else:
            assert np.all(_ends(dsig, SENTINEL) == np.inf)
    acc.close()


@pytest.mark.parametrize("n", [7, 40])
def test_new_points_agree_row_by_row_in_every_chunking(plan, n):
    bt = 2
    _, R = _triangles(n, bt)
    rng = np.random.default_rng(8119500 + n)
    rows = rng.standard_normal((bt, 1000, n))
    pr = rng.uniform(0.5, 2.0, 1000)          # one vector shared by all members
    full = _lev(plan, R, rows, pr, shared=True)["h"]
    for mrows in (1, 63, 64, 65):
        for start in (0, 255, 900):
            part = _lev(plan, R, rows[:, start:start + mrows], pr[start:start + mrows], shared=True)["h"]
            assert np.array_equal(part, full[:, start:start + mrows]), (mrows, start)
    assert np.array_equal(_lev(plan, R, rows, None)["h"] * 1.0, _lev(plan, R, rows, np.ones((bt, 1000)))["h"])


def test_every_info_word_and_untouched_neighbours(plan, qr):
    for m, n in ((16, 8), (100, 33)):
        A, b, p = (v.copy() for v in S.make_case(m, n, True, 5))
        good = _fit(plan, qr, A, b, p, scaled=True)
        A[0][:, 2] = 0.0                      # member 0: a zero column -> 3
        p[1][3] = -1.0                        # member 1: a bad prior -> -1
        p[2][:] = 0.0
        p[2][:n - 1] = 1.0                    # member 2: cnt < n -> -2
        p[3][:] = 0.0
        p[3][:n] = 1.0                        # member 3: dof 0, scaled -> -3
        out = _fit(plan, qr, A, b, p, scaled=True)
        assert list(out["info"]) == [3, -1, -2, -3, 0]
        for k in ("x", "e", "h", "C", "se", "sigma2"):
            assert np.all(out[k][:4] == SENTINEL), k
            assert np.array_equal(out[k][4], good[k][4]), k
        assert np.all(out["dof"][:4] == ISENT)
        un = _fit(plan, qr, A, b, p, scaled=False)
        assert list(un["info"]) == [3, -1, -2, 0, 0] and un["sigma2"][3] == np.inf and un["dof"][3] == 0
        for bad in (NAN, np.inf):
            p2 = p.copy()
            p2[4][m - 1] = bad
            assert _fit(plan, qr, A, b, p2, scaled=False)["info"][4] == -1
    for n in (7, 33):
        bt = 5
        _, R = _triangles(n, bt)
        good = _covar(plan, R)
        jp = np.tile(np.arange(n), (bt, 1))
        rk = np.full(bt, n)
        mult = np.ones(bt)
        R[0][2, 2] = 0.0                      # member 0: a zero diagonal entry -> 3
        jp[1][0] = jp[1][1]                   # member 1: no permutation -> -1
        rk[2] = n + 1                         # member 2: a bad rank -> -1
        mult[3] = -0.5                        # member 3: a bad multiplier -> -1
        out = _covar(plan, R, jp, rk, mult)
        assert list(out["info"]) == [3, -1, -1, -1, 0]
        assert np.all(out["C"][:4] == SENTINEL) and np.all(out["se"][:4] == SENTINEL)
        assert np.array_equal(out["C"][4], good["C"][4]) and np.array_equal(out["se"][4], good["se"][4])
        for v in (NAN, np.inf):
            mult2 = np.ones(bt)
            mult2[4] = v
            assert list(_covar(plan, R, None, None, mult2)["info"]) == [3, 0, 0, 0, -1]
        jp2, rk2 = jp.copy(), np.full(bt, n)
        jp2[1] = np.arange(n)
        jp2[2][n - 1] = n                     # out of range
        rk2[3] = -1
        rk2[0] = 2                            # the zero entry lies past the rank: not an error
        assert list(_covar(plan, R, jp2, rk2, None)["info"]) == [0, 0, -1, -1, 0]
        rows = np.random.default_rng(5).standard_normal((bt, 300, n))
        pr = np.ones((bt, 300))
        pr[4][299] = -1.0                     # a bad prior in the last chunk: no chunk of the member is written
        lev = _lev(plan, R, rows, pr, jpvt=jp, rank=rk)
        assert list(lev["info"]) == [3, -1, -1, 0, -1]
        assert np.all(lev["h"][[0, 1, 2, 4]] == SENTINEL) and np.all(lev["h"][3] != SENTINEL)


@pytest.mark.parametrize("m,n", EXACT, ids=[f"{m}x{n}" for m, n in EXACT])
def test_repeats_batch_independence_and_power_of_two_scaling(plan, qr, m, n):
    A, b, p = S.make_case(m, n, True)
    keys = ("x", "e", "h", "C", "se", "sigma2", "dof", "info")
    base = _fit(plan, qr, A, b, p, scaled=True)
    again = _fit(plan, qr, A, b, p, scaled=True)
    for k in keys:
        assert np.array_equal(base[k], again[k]), k
    sub = _fit(plan, qr, A[[7, 2, 4, 0, 8]], b[[7, 2, 4, 0, 8]], p[[7, 2, 4, 0, 8]], scaled=True)
    one = _fit(plan, qr, A[5:6], b[5:6], p[5:6], scaled=True)
    for k in keys:
        assert np.array_equal(sub[k], base[k][[7, 2, 4, 0, 8]]) and np.array_equal(one[k], base[k][5:6]), k
    few = _fit(plan, qr, A, b, p, scaled=True, want=("se",))
    assert np.array_equal(few["x"], base["x"]) and np.array_equal(few["se"], base["se"])
    un = _fit(plan, qr, A, b, p, scaled=False)
    ua = _fit(plan, qr, A * 8.0, b, p, scaled=False)                       # A 2^k: C 2^-2k, se 2^-k, h unchanged
    assert np.array_equal(ua["C"], un["C"] / 64.0) and np.array_equal(ua["se"], un["se"] / 8.0) and np.array_equal(ua["h"], un["h"])
    sb = _fit(plan, qr, A, b * 0.25, p, scaled=True)                        # b 2^k: x, e 2^k, sigma2 and the scaled C 2^2k
    assert np.array_equal(sb["x"], base["x"] * 0.25) and np.array_equal(sb["e"], base["e"] * 0.25)
    assert np.array_equal(sb["sigma2"], base["sigma2"] / 16.0) and np.array_equal(sb["C"], base["C"] / 16.0)
    assert np.array_equal(sb["h"], base["h"])
    shared = _fit(plan, qr, A, b, p[0], shared=True, scaled=True)
    assert np.array_equal(shared["x"][0], base["x"][0]) and np.array_equal(shared["C"][0], base["C"][0])


def test_host_twin_and_python_wrappers(plan, qr):
    for m, n in ((16, 8), (100, 33)):
        A, b, p = S.make_case(m, n, True, 5)
        dev = _fit(plan, qr, A, b, p, scaled=True)
        out = qr.lstsq_stats_batched(A, b, weights=p, scaled=True)
        assert set(out) == {"x", "resid", "leverage", "sigma2", "dof", "cov", "se", "info"}
        for k, d in (("x", "x"), ("resid", "e"), ("leverage", "h"), ("sigma2", "sigma2"), ("dof", "dof"), ("cov", "C"), ("se", "se"),
                     ("info", "info")):
            assert np.array_equal(out[k], dev[d]), k
        un = qr.lstsq_stats_batched(A, b, scaled=False)
        devu = _fit(plan, qr, A, b, None, scaled=False)
        assert np.array_equal(un["cov"], devu["C"]) and np.array_equal(un["x"], devu["x"])
        # the error path: a member with an info word reads 0 and does not raise
        p2 = p.copy()
        p2[1][0] = -1.0
        bad = qr.lstsq_stats_batched(A, b, weights=p2)
        assert list(bad["info"]) == [0, -1, 0, 0, 0]
        for k in ("x", "resid", "leverage", "sigma2", "dof", "cov", "se"):
            assert np.all(bad[k][1] == 0) and np.array_equal(bad[k][0], out[k][0]), k
    # the twin's own return value: QR_E_SINGULAR where some info word is non-zero, 0 otherwise
    A, b, p = S.make_case(16, 8, True, 5)
    At = np.ascontiguousarray(A.transpose(0, 2, 1))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    X, info = np.empty((5, 8)), np.zeros(5, dtype=np.intc)
    for bad, want in ((False, 0), (True, qr.QR_E_SINGULAR)):
        pw = np.array(p)
        if bad:
            pw[3][2] = NAN
        rc = qr.lib.qr_lstsq_stats_batched(At.ctypes.data_as(dp), 16, 8, np.ascontiguousarray(b).ctypes.data_as(dp), pw.ctypes.data_as(dp),
                                           qr.QR_COV_SCALED, 5, X.ctypes.data_as(dp), None, None, None, None, None, None, info.ctypes.data_as(ip))
        assert rc == want and list(info) == ([0, 0, 0, -1, 0] if bad else [0] * 5)
        assert not bad or np.all(X[3] == 0)
    with pytest.raises(qr.QRError):
        qr.lstsq_stats_batched(np.zeros((2, 3, 4)), np.zeros((2, 3)))
