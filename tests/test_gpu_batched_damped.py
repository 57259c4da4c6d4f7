"""-m gpu: batched damped least squares (mi355x_qr.h section 8f), member by member and lambda by lambda.

Shapes, inputs, truth and measures: tests/batched_damped_ref.py.  The shapes cover the wave route at its register edge ((64,31,1),
(64,28,4)), the first shape past the wave width ((64,32,1): 33 columns), the first past 64 rows ((65,4,1): composed factorisation, wave
solve), the workgroup route up to the LDS limit ((256,63,1)) and a composed one ((300,40,3)).  Every buffer has an odd leading
dimension and an odd stride larger than packed, a base one double off, and is sentinel-filled outside its blocks.

Bound (the rule of test_gpu_range_edges.py): each measure <= min(max(4 x the same measure of the float64 instance of the two-stage
restatement on the same input, eps), cap), the caps of batched_damped_ref.py.  A case that legitimately exceeds 4 x is listed in
MEASURED at twice its measured ratio; the cap holds for it all the same.  The ratios are printed (-s) and tabulated in DESIGN.md
section 7m.
"""
import numpy as np
import pytest
import torch

import batched_damped_ref as D
import hp_ref as H

pytestmark = pytest.mark.gpu

EPS = D.EPS
SENTINEL = -7.25e33
GARBAGE = 123.456

# (call, m, n, nrhs, measure) -> the worst ratio to the float64 restatement over the members and lambdas of the case, measured on an
# MI355X, where it exceeds 4; the bound of such a case is twice the ratio, and never above the cap.  Nearly all
# of them are figures of one or two eps set against a restatement that happened to round to a tenth of an eps on the same input.
MEASURED = {
    ('gels_damped', 1, 1, 1, 'forward'): 21.3,
    ('gels_damped', 1, 1, 1, 'xnorm'): 26.4,
    ('gels_damped', 5, 3, 2, 'resid'): 6.82,
    ('gels_damped', 5, 3, 2, 'xnorm'): 16.7,
    ('gels_damped', 17, 17, 1, 'forward'): 7.17,
    ('gels_damped', 17, 17, 1, 'resid'): 5.78,
    ('gels_damped', 17, 17, 1, 'xnorm'): 38,
    ('gels_damped', 64, 28, 4, 'xnorm'): 4.06,
    ('gels_damped', 64, 31, 1, 'resid'): 7.79,
    ('gels_damped', 64, 31, 1, 'xnorm'): 26.6,
    ('gels_damped', 64, 32, 1, 'resid'): 5.58,
    ('gels_damped', 64, 32, 1, 'xnorm'): 9.39,
    ('gels_damped', 65, 4, 1, 'forward'): 4.76,
    ('gels_damped', 65, 4, 1, 'xnorm'): 77.6,
    ('gels_damped', 256, 63, 1, 'xnorm'): 22.7,
    ('gels_damped_noD', 5, 3, 2, 'forward'): 6.02,
    ('gels_damped_noD', 5, 3, 2, 'xnorm'): 4.24,
    ('gels_damped_noD', 64, 28, 4, 'xnorm'): 7.51,
    ('gels_damped_wide', 1, 2, 1, 'resid'): 4.13,
    ('gels_damped_wide', 1, 2, 1, 'xnorm'): 5.71,
    ('gels_damped_wide', 1, 2, 3, 'forward'): 4.13,
    ('gels_damped_wide', 1, 2, 3, 'xnorm'): 5.12,
    ('gels_damped_wide', 3, 31, 3, 'resid'): 4.73,
    ('gels_damped_wide', 6, 7, 1, 'resid'): 13.1,
    ('gels_damped_wide', 6, 7, 1, 'xnorm'): 47.7,
    ('gels_damped_wide', 6, 7, 3, 'resid'): 4.91,
    ('gels_damped_wide', 6, 7, 3, 'xnorm'): 5.09,
    ('gels_damped_wide', 8, 64, 1, 'resid'): 19.8,
    ('gels_damped_wide', 33, 100, 3, 'resid'): 4.22,
    ('gels_damped_wide', 40, 300, 1, 'resid'): 76.6,
}


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


def _odd(x):
    return x + 3 - x % 2


class Strided:
    """`batch` column-major blocks of rows x cols at an odd leading dimension > rows and an odd stride > ld * cols, the base one
    element off; everything outside the blocks holds SENTINEL"""

    def __init__(self, rows, cols, batch, fill=None, dtype=np.float64):
        self.shape = (batch, rows, cols)
        self.ld = _odd(rows)
        self.stride = _odd(self.ld * cols + 4)
        self.init = np.full(1 + batch * self.stride, SENTINEL if dtype == np.float64 else -77, dtype=dtype)
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
        return np.array_equal(self.t.cpu().numpy(), self.init)


class Shared:
    """one block of `len` values for every member: stride 0"""

    def __init__(self, v):
        self.t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()
        self.ptr, self.stride = self.t, 0


def _vec(v, shared):
    """per-member vectors v (batch, len), or None; shared: member 0's for everybody, at stride 0"""
    if v is None:
        return None
    return Shared(v[0]) if shared else Strided(v.shape[1], 1, v.shape[0], v[:, :, None])


class Out:
    """X, xnorm, resid, info of one call, sentinel-filled"""

    def __init__(self, xrows, nrhs, nlam, b):
        self.b, self.nrhs, self.nlam = b, nrhs, nlam
        self.X = Strided(xrows, nlam * nrhs, b)
        self.xn = torch.full((b * nlam * nrhs,), SENTINEL, dtype=torch.float64, device="cuda")
        self.rs = torch.full((b * nlam * nrhs,), SENTINEL, dtype=torch.float64, device="cuda")
        self.info = torch.full((b * nlam,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def collect(self):
        b, nrhs, nlam = self.b, self.nrhs, self.nlam
        X = self.X.get()
        rows = X.shape[1]
        return dict(X=X.reshape(b, rows, nlam, nrhs).transpose(0, 2, 1, 3).copy(),          # (b, nlam, rows, nrhs)
                    xnorm=self.xn.cpu().numpy().reshape(b, nlam, nrhs), resid=self.rs.cpu().numpy().reshape(b, nlam, nrhs),
                    info=self.info.cpu().numpy().reshape(b, nlam))


def _opt(x):
    return (None, 0) if x is None else (x.ptr, x.stride)


def _fused(plan, A, B, d, lam, shared=False):
    """qr_gels_damped_batched_dev: the results, and the factors and Q^T B it leaves"""
    b, m, n = A.shape
    nrhs, nlam = B.shape[2], lam.shape[1]
    dA, dtau, dB = Strided(m, n, b, A), Strided(n, 1, b), Strided(m, nrhs, b, B)
    dD, dl, o = _vec(d, shared), _vec(lam, shared), Out(n, nrhs, nlam, b)
    Dp, Ds = _opt(dD)
    plan.gels_damped_batched(dA.ptr, m, n, dA.ld, dA.stride, dtau.ptr, dtau.stride, dB.ptr, nrhs, dB.ld, dB.stride, dl.ptr, nlam, dl.stride,
                             o.X.ptr, o.X.ld, o.X.stride, o.info, b, dD=Dp, strideD=Ds, dxnorm=o.xn, dresid=o.rs)
    plan.sync()
    out = o.collect()
    out.update(F=dA.get(), tau=dtau.get()[:, :, 0], QtB=dB.get())
    return out


def _damped(plan, R, Z, d, lam, rss=None, jpvt=None, flip=False, shared=False):
    """qr_damped_batched_dev on R (batch, n, n; what lies below the diagonal is not read) and Z (batch, n, nrhs)"""
    b, n, _ = R.shape
    nrhs, nlam = Z.shape[2], lam.shape[1]
    dR, dZ = Strided(n, n, b, R), Strided(n, nrhs, b, Z)
    dD, dl, o = _vec(d, shared), _vec(lam, shared), Out(n, nrhs, nlam, b)
    drss = None if rss is None else torch.from_numpy(np.ascontiguousarray(rss)).cuda()
    dj = None if jpvt is None else Strided(n, 1, b, jpvt[:, :, None].astype(np.int32), dtype=np.int32)
    Dp, Ds = _opt(dD)
    Jp, Js = _opt(dj)
    plan.damped_batched(dR.ptr, n, dR.ld, dR.stride, dZ.ptr, nrhs, dZ.ld, dZ.stride, dl.ptr, nlam, dl.stride, o.X.ptr, o.X.ld, o.X.stride,
                        o.info, b, drss=drss, djpvt=Jp, stridejpvt=Js, dD=Dp, strideD=Ds, flip=flip, dxnorm=o.xn, dresid=o.rs)
    plan.sync()
    assert dR.unchanged() and dZ.unchanged(), "the factors are read only"
    return o.collect()


def _wide(plan, A, B, lam):
    """qr_gels_damped_wide_batched_dev on the wide members A (batch, m, n), m < n"""
    b, m, n = A.shape
    nrhs, nlam = B.shape[2], lam.shape[1]
    dA, dF, dtau, dB = Strided(m, n, b, A), Strided(n, m, b), Strided(m, 1, b), Strided(m, nrhs, b, B)
    dl, o = _vec(lam, False), Out(n, nrhs, nlam, b)
    plan.gels_damped_wide_batched(dA.ptr, m, n, dA.ld, dA.stride, dF.ptr, dF.ld, dF.stride, dtau.ptr, dtau.stride, dB.ptr, nrhs, dB.ld,
                                  dB.stride, dl.ptr, nlam, dl.stride, o.X.ptr, o.X.ld, o.X.stride, o.info, b, dxnorm=o.xn, dresid=o.rs)
    plan.sync()
    assert dA.unchanged() and dB.unchanged(), "the wide matrix, the right-hand sides and their padding are untouched"
    out = o.collect()
    out.update(F=dF.get(), tau=dtau.get()[:, :, 0])
    return out


def _gels(plan, A, B):
    b, m, n = A.shape
    nrhs = B.shape[2]
    dA, dtau, dB = Strided(m, n, b, A), Strided(n, 1, b), Strided(m, nrhs, b, B)
    info = torch.full((b,), 77, dtype=torch.int32, device="cuda")
    plan.gels_batched(dA.ptr, m, n, dA.ld, dA.stride, dtau.ptr, dtau.stride, dB.ptr, nrhs, dB.ld, dB.stride, info, b)
    plan.sync()
    return dict(F=dA.get(), tau=dtau.get()[:, :, 0], B=dB.get(), info=info.cpu().numpy())


def _within(tag, key, got, ref, cap):
    """prints the figure and its bound; returns whether the figure is inside"""
    factor = 2.0 * MEASURED[key] if key in MEASURED else 4.0
    bound = min(max(factor * ref, EPS), cap)
    ok = bool(np.isfinite(got) and got <= bound)
    print(f"RATIO {tag}: {got:.3e} is {got / max(ref, EPS / 4):.2f} x the float64 reference {ref:.3e}; bound {bound:.3e} (cap {cap:.3e})"
          + ("" if ok else "  OUTSIDE"))
    return ok


def _check(call, shape, c, out, units):
    """every (member, lambda)'s four measures against the rule, every figure printed before the one assertion; the key of MEASURED is
    (call, m, n, nrhs, measure): the worst ratio over the members and the lambdas of a case"""
    worst, outside = np.zeros(4), []
    for q in range(len(c["A"])):
        dq = None if c["d"] is None else c["d"][q]
        for k, lam in enumerate(c["lam"][q]):
            got = D.measures(c["A"][q], c["B"][q], lam, dq, out["X"][q, k], out["xnorm"][q, k], out["resid"][q, k], c["T"][q][k])
            for i, name in enumerate(D.NAMES):
                worst[i] = max(worst[i], got[i] / max(c["ref"][q][k][i], EPS / 4))
                tag = f"{call} {shape} member {q} lambda {units[k]:g} {name}"
                if not _within(tag, (call,) + shape + (name,), got[i], c["ref"][q][k][i], c["caps"][q][k][i]):
                    outside.append(tag)
    for n, w in zip(D.NAMES, worst):
        print(f"WORST {call} {shape} {n} {w:.2f}")
    assert not outside, outside


def _units(m, n):
    return [l for l in D.LAMS if l > 0 or m > n]


# ------------------------------------------------------------------------------------------------
# accuracy, every shape, as one list and one lambda at a time
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", D.SHAPES)
def test_accuracy_against_the_longdouble_truth(plan, m, n, nrhs):
    c = D.case(m, n, nrhs)
    out = _fused(plan, c["A"], c["B"], c["d"], c["lam"])
    assert np.all(out["info"] == 0)
    _check("gels_damped", (m, n, nrhs), c, out, _units(m, n))
    for k in range(c["lam"].shape[1]):       # a lambda alone is the same lambda inside the list, bit for bit
        one = _fused(plan, c["A"], c["B"], c["d"], c["lam"][:, k:k + 1])
        for key in ("X", "xnorm", "resid", "info"):
            assert np.array_equal(one[key][:, 0], out[key][:, k]), (key, k)


@pytest.mark.parametrize("m,n,nrhs", [(5, 3, 2), (64, 28, 4), (100, 33, 2)])
def test_accuracy_without_d(plan, m, n, nrhs):
    c = D.case(m, n, nrhs, False)
    out = _fused(plan, c["A"], c["B"], None, c["lam"])
    assert np.all(out["info"] == 0)
    _check("gels_damped_noD", (m, n, nrhs), c, out, _units(m, n))


# ------------------------------------------------------------------------------------------------
# lambda = 0 on the wave route is qr_gels_batched_dev, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", [(5, 3, 2), (64, 31, 1), (64, 28, 4)])
def test_lambda_zero_on_the_wave_route_is_gels_bitwise(plan, m, n, nrhs):
    c = D.case(m, n, nrhs)
    lam = np.zeros((len(c["A"]), 1))
    out = _fused(plan, c["A"], c["B"], c["d"], lam)
    g = _gels(plan, c["A"], c["B"])
    assert np.all(out["info"] == 0) and np.all(g["info"] == 0)
    assert np.array_equal(out["X"][:, 0], g["B"][:, :n])
    assert np.array_equal(out["F"], g["F"]) and np.array_equal(out["tau"], g["tau"])
    assert np.array_equal(out["QtB"][:, n:], g["B"][:, n:]), "the tail rows of Q^T B"


# ------------------------------------------------------------------------------------------------
# the fused call equals the solve from the factors it left, on every route
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", [(5, 3, 2), (64, 28, 4), (64, 32, 1), (65, 4, 1), (100, 33, 2), (256, 63, 1), (300, 40, 3)])
def test_fused_equals_the_solve_from_its_own_outputs(plan, m, n, nrhs):
    c = D.case(m, n, nrhs)
    out = _fused(plan, c["A"], c["B"], c["d"], c["lam"])
    rss = (out["QtB"][:, n:] ** 2).sum(axis=1)
    again = _damped(plan, out["F"][:, :n], out["QtB"][:, :n], c["d"], c["lam"], rss)
    assert np.all(again["info"] == 0)
    assert np.array_equal(again["X"], out["X"]) and np.array_equal(again["xnorm"], out["xnorm"])
    assert np.allclose(again["resid"], out["resid"], rtol=64 * EPS, atol=0)     # (rss is summed in another order)


# ------------------------------------------------------------------------------------------------
# repeats, batch count, index, shared lambda and d
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", [(64, 28, 4), (64, 32, 1), (100, 33, 2)])
def test_repeatable_and_independent_of_batch_and_index(plan, m, n, nrhs):
    c = D.case(m, n, nrhs, True, 9)
    keys = ("X", "xnorm", "resid", "info", "F", "tau", "QtB")
    a, b = _fused(plan, c["A"], c["B"], c["d"], c["lam"]), _fused(plan, c["A"], c["B"], c["d"], c["lam"])
    for k in keys:
        assert np.array_equal(a[k], b[k]), k
    for q in (0, 3, 8):                   # members of full workgroups and of the ragged last one, each alone
        one = _fused(plan, c["A"][q:q + 1], c["B"][q:q + 1], c["d"][q:q + 1], c["lam"][q:q + 1])
        for k in keys:
            assert np.array_equal(one[k][0], a[k][q]), (k, q)
    rev = _fused(plan, c["A"][::-1], c["B"][::-1], c["d"][::-1], c["lam"][::-1])
    for k in keys:
        assert np.array_equal(rev[k][::-1], a[k]), k
    # one lambda list and one d for everybody: stride 0 equals the replicated arrays
    lam0, d0 = np.repeat(c["lam"][:1], 9, axis=0), np.repeat(c["d"][:1], 9, axis=0)
    rep, sh = _fused(plan, c["A"], c["B"], d0, lam0), _fused(plan, c["A"], c["B"], d0, lam0, shared=True)
    for k in keys:
        assert np.array_equal(rep[k], sh[k]), k


# ------------------------------------------------------------------------------------------------
# scaling by a power of two is exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs", [(64, 28, 4), (100, 33, 2)])
def test_scale_equivariance_is_exact(plan, m, n, nrhs):
    c = D.case(m, n, nrhs, True, 5)
    A, B, d, lam = c["A"], c["B"], c["d"], c["lam"][:, 1:]       # (lambda = 0 scales trivially)
    base = _fused(plan, A, B, d, lam)
    for k in (40, -40):
        s = 2.0 ** k
        o = _fused(plan, s * A, B, d, s * lam)
        assert np.array_equal(o["X"], base["X"] / s), ("(A, lambda) scaled", k)
        assert np.array_equal(o["resid"], base["resid"]) and np.array_equal(o["xnorm"], base["xnorm"] / s)
        o = _fused(plan, A, s * B, d, lam)
        for key in ("X", "xnorm", "resid"):
            assert np.array_equal(o[key], base[key] * s), ("B scaled", key, k)
        o = _fused(plan, A, B, s * d, lam / s)
        assert np.array_equal(o["X"], base["X"]) and np.array_equal(o["resid"], base["resid"]), ("D 2^k, lambda 2^-k", k)
        assert np.array_equal(o["xnorm"], base["xnorm"] * s)


# ------------------------------------------------------------------------------------------------
# the info word: a pair fails alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,nrhs,zero", [(64, 28, 4, 11), (100, 33, 2, 0), (300, 40, 3, 39)])
def test_a_zero_column_with_a_zero_d_fails_its_pair_alone(plan, m, n, nrhs, zero):
    c = D.case(m, n, nrhs, True, 5)
    lam = np.ascontiguousarray(c["lam"][:, 2:5])
    A, d = c["A"].copy(), np.repeat(c["d"][:, None, :], 3, axis=1).copy()        # d per (member, lambda): three calls of one lambda
    A[1][:, zero] = 0.0
    good = [_fused(plan, A, c["B"], c["d"], lam[:, k:k + 1]) for k in range(3)]
    d[1, 1, zero] = 0.0                   # for lambda 1 of member 1 only
    bad = _fused(plan, A, c["B"], d[:, 1], lam[:, 1:2])
    info = np.zeros((5, 1), dtype=int)
    info[1, 0] = zero + 1
    assert np.array_equal(bad["info"], info)
    assert np.all(bad["X"][1] == SENTINEL) and np.all(bad["xnorm"][1] == SENTINEL) and np.all(bad["resid"][1] == SENTINEL)
    for q in (0, 2, 3, 4):
        for key in ("X", "xnorm", "resid"):
            assert np.array_equal(bad[key][q], good[1][key][q]), (key, q)
    # the same column at lambda = 0 inside a list of three: one pair fails, its neighbours are bitwise the single calls
    lam0 = lam.copy()
    lam0[1, 1] = 0.0
    mixed = _fused(plan, A, c["B"], c["d"], lam0)
    info3 = np.zeros((5, 3), dtype=int)
    info3[1, 1] = zero + 1
    assert np.array_equal(mixed["info"], info3)
    assert np.all(mixed["X"][1, 1] == SENTINEL) and np.all(mixed["xnorm"][1, 1] == SENTINEL) and np.all(mixed["resid"][1, 1] == SENTINEL)
    for q in range(5):
        for k in range(3):
            if (q, k) != (1, 1):
                for key in ("X", "xnorm", "resid"):
                    assert np.array_equal(mixed[key][q, k], good[k][key][q, 0]), (key, q, k)


# ------------------------------------------------------------------------------------------------
# pivoted factors
# ------------------------------------------------------------------------------------------------
def test_pivoted_factors_of_rank_deficient_members(plan):
    b, m, n, nrhs, r = 5, 64, 28, 2, 5
    A = np.stack([D.U(900 + q, m, r) @ D.U(950 + q, r, n) for q in range(b)])
    B, d = D.U(990, b, m, nrhs), 0.5 + 1.5 * np.random.default_rng(991).random((b, n))
    lam = np.stack([np.array([0.3, 1e-8]) * np.linalg.norm(A[q], 2) for q in range(b)])
    dA, dtau, dj = Strided(m, n, b, A), Strided(n, 1, b), Strided(n, 1, b, dtype=np.int32)
    plan.geqp3_batched(dA.ptr, m, n, dA.ld, dA.stride, dj.ptr, dj.stride, dtau.ptr, dtau.stride, b)
    dB = Strided(m, nrhs, b, B)
    plan.ormqr_batched("T", dA.ptr, m, n, dA.ld, dA.stride, dtau.ptr, dtau.stride, dB.ptr, nrhs, dB.ld, dB.stride, b)
    plan.sync()
    F, QtB, jp = dA.get(), dB.get(), dj.get()[:, :, 0]
    out = _damped(plan, F[:, :n], QtB[:, :n], d, lam, (QtB[:, n:] ** 2).sum(axis=1), jpvt=jp)
    assert np.all(out["info"] == 0)
    for q in range(b):
        for k in range(2):
            t = D.truth(A[q], B[q], lam[q, k], d[q])
            got = D.measures(A[q], B[q], lam[q, k], d[q], out["X"][q, k], out["xnorm"][q, k], out["resid"][q, k], t)
            cp = D.caps(A[q], B[q], lam[q, k], d[q], t)
            print(f"RATIO pivoted member {q} lambda {k}: " + ", ".join(f"{nm} {g:.3e} (cap {c:.3e})" for nm, g, c in zip(D.NAMES, got, cp)))
            for g, cap in zip(got, cp):
                assert np.isfinite(g) and g <= cap


# ------------------------------------------------------------------------------------------------
# the accumulator
# ------------------------------------------------------------------------------------------------
def _acc_state(acc):
    return [np.array(x) for x in acc.factor_host()]


def _acc_solve_damped(acc, plan, n, nrhs, b, d, lam):
    nlam = lam.shape[1]
    dD, dl, o = _vec(d, False), _vec(lam, False), Out(n, nrhs, nlam, b)
    Dp, Ds = _opt(dD)
    acc.solve_damped(dl.ptr, nlam, dl.stride, o.X.ptr, o.X.ld, o.X.stride, o.info, dD=Dp, strideD=Ds, dxnorm=o.xn, dresid=o.rs)
    plan.sync()
    return o.collect()


def test_accumulator_solves_damped_and_keeps_its_state(qr, plan):
    b, n, nrhs, m = 5, 8, 2, 40
    c = D.case(m, n, nrhs, True, b)
    lam = np.ascontiguousarray(c["lam"][:, 2:4])                  # lambda > 0
    acc = qr.LsAccumulatorBatched(plan, n, nrhs, b)
    try:
        s0 = _acc_state(acc)
        out = _acc_solve_damped(acc, plan, n, nrhs, b, c["d"], lam)
        assert np.all(out["info"] == 0) and np.all(out["X"] == 0) and np.all(out["xnorm"] == 0) and np.all(out["resid"] == 0)
        assert all(np.array_equal(x, y) for x, y in zip(s0, _acc_state(acc)))
        # three rows: fewer than n, solvable for lambda > 0
        dA, dB = Strided(m, n, b, c["A"]), Strided(m, nrhs, b, c["B"])
        acc.push(dA.ptr, 3, dA.ld, dA.stride, dB.ptr, dB.ld, dB.stride)
        plan.sync()
        s1 = _acc_state(acc)
        out = _acc_solve_damped(acc, plan, n, nrhs, b, c["d"], lam)
        assert np.all(out["info"] == 0) and all(np.array_equal(x, y) for x, y in zip(s1, _acc_state(acc)))
        for q in range(b):
            for k in range(2):
                A3, B3 = c["A"][q][:3], c["B"][q][:3]
                t = D.truth(A3, B3, lam[q, k], c["d"][q])
                got = D.measures(A3, B3, lam[q, k], c["d"][q], out["X"][q, k], out["xnorm"][q, k], out["resid"][q, k], t)
                cp = D.caps(A3, B3, lam[q, k], c["d"][q], t)
                print(f"RATIO accumulator 3 rows member {q} lambda {k}: " + ", ".join(f"{nm} {g:.3e} (cap {x:.3e})" for nm, g, x in zip(D.NAMES, got, cp)))
                assert all(np.isfinite(g) and g <= x for g, x in zip(got, cp))
        # the full window: against the fused call on the same rows
        ptr = dA.ptr[3:]
        acc.push(ptr, m - 3, dA.ld, dA.stride, dB.ptr[3:], dB.ld, dB.stride)
        plan.sync()
        s2 = _acc_state(acc)
        lam0 = np.concatenate([np.zeros((b, 1)), lam], axis=1)
        out = _acc_solve_damped(acc, plan, n, nrhs, b, c["d"], lam0)
        assert np.all(out["info"] == 0) and all(np.array_equal(x, y) for x, y in zip(s2, _acc_state(acc)))
        fused = _fused(plan, c["A"], c["B"], c["d"], lam0)
        for q in range(b):
            for k in range(3):
                cap = c["caps"][q][0 if k == 0 else k + 1]
                e = np.linalg.norm(out["X"][q, k] - fused["X"][q, k]) / np.linalg.norm(fused["X"][q, k])
                print(f"RATIO accumulator window member {q} lambda {k}: against the fused call {e:.3e} (cap {cap[0]:.3e})")
                assert e <= cap[0]
                assert np.allclose(out["resid"][q, k], fused["resid"][q, k], rtol=cap[2]) and np.allclose(out["xnorm"][q, k], fused["xnorm"][q, k], rtol=cap[1])
        # lambda = 0 is qr_lsacc_batched_solve_dev, bit for bit
        dX = Strided(n, nrhs, b)
        info = torch.full((b,), 77, dtype=torch.int32, device="cuda")
        acc.solve(dX.ptr, dX.ld, dX.stride, info)
        plan.sync()
        assert np.all(info.cpu().numpy() == 0) and np.array_equal(dX.get(), out["X"][:, 0])
    finally:
        acc.close()


# ------------------------------------------------------------------------------------------------
# wide members, D = I
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrhs", D.WIDE_NRHS)
@pytest.mark.parametrize("rows,cols", D.WIDE)
def test_wide_members_against_the_truth(plan, rows, cols, nrhs):
    m, n = cols, rows                     # the member is the transpose of the tall F-shape
    c = D.case(m, n, nrhs, False, 5)
    lam = np.ascontiguousarray(c["lam"][:, :3])
    out = _wide(plan, c["A"], c["B"], lam)
    assert np.all(out["info"] == 0)
    c3 = dict(c, lam=lam)
    _check("gels_damped_wide", (m, n, nrhs), c3, out, _units(m, n)[:3])
    # as lambda -> 1e-8 |A|_2 the result approaches the minimum-norm solution of qr_gels_wide_batched_dev within the cap
    dA, dF, dtau = Strided(m, n, 5, c["A"]), Strided(n, m, 5), Strided(m, 1, 5)
    img = np.zeros((5, n, nrhs))
    img[:, :m] = c["B"]
    dB = Strided(n, nrhs, 5, img)
    info = torch.full((5,), 77, dtype=torch.int32, device="cuda")
    plan.gels_wide_batched(dA.ptr, m, n, dA.ld, dA.stride, dF.ptr, dF.ld, dF.stride, dtau.ptr, dtau.stride, dB.ptr, nrhs, dB.ld, dB.stride, info, 5)
    plan.sync()
    Xm = dB.get()
    for q in range(5):
        e = np.linalg.norm(out["X"][q, 0] - Xm[q]) / np.linalg.norm(Xm[q])
        bound = c["caps"][q][0][0] + (1e-8 * np.linalg.cond(c["A"][q])) ** 2       # (the damping moves x by (lambda / sigma_min)^2 at most)
        print(f"RATIO wide {m}x{n} member {q}: against the minimum-norm solution {e:.3e} (bound {bound:.3e})")
        assert e <= bound


# ------------------------------------------------------------------------------------------------
# host pointers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,with_d", [(20, 7, True), (100, 33, False), (6, 7, False), (33, 100, False)])
def test_host_twin_matches_numpy(qr, m, n, with_d):
    b, nrhs = 5, 3
    A, B = D.U(m * n, b, m, n), D.U(m * n + 1, b, m, nrhs)
    d = (0.5 + 1.5 * np.random.default_rng(3).random((b, n))) if with_d else None
    lam = np.stack([np.array([1e-8, 0.3, 30.0]) * np.linalg.norm(A[q], 2) for q in range(b)])
    A0, B0 = A.copy(), B.copy()
    X, xnorm, resid, info = qr.lstsq_damped_batched(A, B, lam, d)
    assert X.shape == (b, 3, n, nrhs) and np.all(info == 0) and np.array_equal(A, A0) and np.array_equal(B, B0)
    for q in range(b):
        dd = np.ones(n) if d is None else d[q]
        for k in range(3):
            S = np.vstack([A[q], lam[q, k] * np.diag(dd)])
            C = np.vstack([B[q], np.zeros((n, nrhs))])
            Xn = np.linalg.lstsq(S, C, rcond=None)[0]
            kappa = np.linalg.cond(S)
            bound = 50 * (kappa + kappa ** 2 * np.linalg.norm(S @ Xn - C) / (np.linalg.norm(S, 2) * np.linalg.norm(Xn))) * EPS
            e = np.linalg.norm(X[q, k] - Xn) / np.linalg.norm(Xn)
            print(f"lstsq_damped_batched {m}x{n} member {q} lambda {k}: against numpy {e:.3e} (bound {bound:.3e})")
            assert e <= bound
            assert np.allclose(xnorm[q, k], np.linalg.norm(dd[:, None] * Xn, axis=0), rtol=4 * bound + n * EPS)
            rn = np.linalg.norm(A[q] @ Xn - B[q], axis=0)
            assert np.all(np.abs(resid[q, k] - rn) <= bound * np.linalg.norm(A[q], 2) * np.linalg.norm(Xn) + (m + n) * EPS * rn)


def test_host_twin_reports_a_singular_pair(qr):
    b, m, n = 4, 12, 5
    A, B = D.U(71, b, m, n), D.U(72, b, m, 2)
    A[2][:, 3] = 0.0
    lam = np.tile(np.array([0.0, 0.5]), (b, 1))
    X, xnorm, resid, info = qr.lstsq_damped_batched(A, B, lam)
    assert np.array_equal(info, [[0, 0], [0, 0], [4, 0], [0, 0]])
    Xn = np.linalg.lstsq(np.vstack([A[2], 0.5 * np.eye(n)]), np.vstack([B[2], np.zeros((n, 2))]), rcond=None)[0]
    assert np.linalg.norm(X[2, 1] - Xn) <= 1e-12 * np.linalg.norm(Xn)


# ------------------------------------------------------------------------------------------------
# flip on a bare triangle
# ------------------------------------------------------------------------------------------------
def test_flip_alone_equals_the_restatement(plan):
    """qr_damped_batched_dev with flip on a bare triangle, both routes: against the float64 restatement's own accuracy"""
    for n, nrhs in ((6, 2), (40, 3)):
        b = 5
        R = np.triu(D.U(n, b, n, n)) + 2.0 * np.eye(n)
        Z = D.U(n + 1, b, n, nrhs)
        lam = np.tile(np.array([0.25, 3.0]), (b, 1))
        out = _damped(plan, R + np.tril(np.full((n, n), GARBAGE), -1), Z, None, lam, flip=True)
        assert np.all(out["info"] == 0)
        for q in range(b):
            for k in range(2):
                Xl, xl, rl, _ = D.solve(R[q], Z[q], lam[q, k], flip=True, dtype=D.LD)
                X64, _, _, _ = D.solve(R[q], Z[q], lam[q, k], flip=True)
                ref = float(H.norm(H.arr(X64) - Xl) / H.norm(Xl))
                got = float(H.norm(H.arr(out["X"][q, k]) - Xl) / H.norm(Xl))
                kap = np.linalg.cond(np.vstack([R[q], lam[q, k] * np.eye(n)]))
                print(f"RATIO flip n={n} member {q} lambda {k}: {got:.3e} against the restatement's {ref:.3e}")
                assert got <= min(max(4 * ref, EPS), 50 * kap * EPS)
                assert abs(out["xnorm"][q, k, 0] - float(xl[0])) <= 50 * kap * EPS * float(xl[0])
