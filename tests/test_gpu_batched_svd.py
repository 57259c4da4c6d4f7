"""-m gpu: the batched SVD of small matrices (mi355x_qr.h section 8c), matrix by matrix.

Shapes, input classes and bounds are those of batched_svd_ref.py (the smallest shapes that reach both routes, the last n of the wave
route and the first of the workgroup route, odd n, the LDS edges; batch 5, no multiple of four).  With s = a matrix's reported sweeps
and unit = s n eps (test_gpu_svd.py) and (n + 8) eps for the factorisation's own share (test_gpu_batched.py):

    |A - U S V^T| / |A| <= unit + (n + 8) eps       max |sigma_i - sigma_i(numpy)| / sigma_0 <= unit + (n + 8) eps
    |V^T V - I| <= 4 unit                           |U^T U - I| <= 4 unit + (n + 8) eps       (all n columns, rank-deficient inputs too)

and the sweeps are at most those of the numpy restatement on the same device-computed R and jpvt, plus 2 for the different order of
the sums.

Observed on an MI355X, over all shapes (sweeps include the idle last one): Gaussian 1 to 10 sweeps, condition 1e6 1 to 9, condition
1e12 1 to 8, exact ranks 1 to 9, zero plus duplicated column 1 to 9, the zero matrix and the identity 1, mixed batches 1 to 10, 16 x 8
x 1100 1 to 7; never more than the restatement's count plus 1, every rank exact, and the four errors at 0.29 of their bounds or less
(the largest: |U^T U - I| at n = 64).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import batched_svd_ref as B

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = -7.25e33


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # deliberately small: the batched calls take the plan's stream, not its shape
    yield p
    p.close()


def _up(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    return t


def _down(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def _pack(A):
    return np.ascontiguousarray(A.transpose(0, 2, 1))


def _ints(*shape, fill=-9):
    return _up(np.full(shape, fill, dtype=np.int32))


def _svd(plan, A, jobu="U", jobv="V"):
    """the packed call; returns a dict of everything it left: U (batch, m, n), S, V (batch, n, n), rank, sweeps, info, F, tau, jpvt"""
    batch, m, n = A.shape
    dA, dtau, dj = _up(_pack(A)), _up(np.full((batch, n), SENTINEL)), _ints(batch, n)
    dS, dinfo, drank, dsw = _up(np.full((batch, n), SENTINEL)), _ints(batch), _ints(batch), _ints(batch)
    dU = _up(np.full((batch, n, m), SENTINEL)) if jobu == "U" else None
    dV = _up(np.full((batch, n, n), SENTINEL)) if jobv == "V" else None
    plan.gesvd_batched(jobu, jobv, dA, m, n, m, m * n, dj, n, dtau, n, dS, n, dinfo, batch, dU=dU, ldu=m, strideU=m * n, dV=dV, ldv=n,
                       strideV=n * n, drank=drank, dsweeps=dsw)
    plan.sync()
    return dict(U=_down(dU).transpose(0, 2, 1) if dU is not None else None, S=_down(dS), V=_down(dV).transpose(0, 2, 1) if dV is not None else None,
                rank=_down(drank).astype(np.int64), sweeps=_down(dsw).astype(np.int64), info=_down(dinfo).astype(np.int64),
                F=_down(dA).transpose(0, 2, 1), tau=_down(dtau), jpvt=_down(dj).astype(np.int64))


def _same(x, y, keys=("U", "S", "V", "rank", "sweeps", "info", "F", "tau", "jpvt")):
    return all(np.array_equal(x[k], y[k]) for k in keys if x[k] is not None)


@functools.lru_cache(maxsize=None)
def _ref_sweeps(key):
    """the restatement's sweeps on the R and jpvt the device computed (key: the bytes of both)"""
    Rb, jb, n = key
    R = np.frombuffer(Rb).reshape(n, n)
    return B.jsvd_ref(R, np.frombuffer(jb, dtype=np.int64), want_w=False)[4]


def _check(A, out, ranks=None, tag=""):
    batch, m, n = A.shape
    assert np.all(out["info"] == 0)
    assert np.all(np.isfinite(out["U"])) and np.all(np.isfinite(out["V"])) and np.all(np.isfinite(out["S"]))
    worst, got, ref = np.zeros(4), [], []
    for q in range(batch):
        S, sw, rk = out["S"][q], int(out["sweeps"][q]), int(out["rank"][q])
        worst = np.maximum(worst, B.check_bounds(A[q], out["U"][q], S, out["V"][q], sw))
        assert np.all(S[rk:] == 0.0) and np.all(S[:rk] > 0.0)
        if ranks is not None:
            assert rk == ranks[q], (q, rk, ranks[q])
        R = np.triu(out["F"][q][:n])
        rs = _ref_sweeps((R.tobytes(), out["jpvt"][q].tobytes(), n))
        got.append(sw)
        ref.append(rs)
    print(f"batched svd {tag} {m}x{n}: sweeps {got} (restatement {ref}), fractions of the bounds (rec, sigma, V, U) {np.round(worst, 3)}")
    for sw, rs in zip(got, ref):
        assert 1 <= sw <= rs + 2, (got, ref)


@pytest.mark.parametrize("kind,m,n", B.cases())
def test_every_class_at_every_shape(qr, plan, kind, m, n):
    A, ranks = B.make_batch(kind, m, n)
    out = _svd(plan, A)
    _check(A, out, ranks, kind)
    # dA, dtau and djpvt are what qr_geqp3_batched_dev alone leaves, bit for bit
    dA, dtau, dj = _up(_pack(A)), _up(np.full((B.BATCH, n), SENTINEL)), _ints(B.BATCH, n)
    plan.geqp3_batched(dA, m, n, m, m * n, dj, n, dtau, n, B.BATCH)
    plan.sync()
    assert np.array_equal(_down(dA).transpose(0, 2, 1), out["F"]) and np.array_equal(_down(dtau), out["tau"])
    assert np.array_equal(_down(dj), out["jpvt"])
    # values only: the same S, rank and sweeps, bit for bit; each output alone too
    for ju, jv in (("N", "N"), ("U", "N"), ("N", "V")):
        o2 = _svd(plan, A, ju, jv)
        assert _same(o2, out, ("S", "rank", "sweeps", "info", "F", "tau", "jpvt")), (ju, jv)
        assert o2["U"] is None or np.array_equal(o2["U"], out["U"])
        assert o2["V"] is None or np.array_equal(o2["V"], out["V"])
    assert _same(_svd(plan, A), out)                                           # a repeat call


def test_more_matrices_than_compute_units(qr, plan):
    m, n, batch = 16, 8, 1100
    rng = np.random.default_rng(168)
    A = rng.standard_normal((batch, m, n))
    A[3] = B.with_rank(rng, m, n, 3)
    A[batch - 1] = 0.0
    A[batch - 2] = A[0]
    out = _svd(plan, A)
    assert np.all(out["info"] == 0)
    assert out["rank"][3] == 3 and out["rank"][batch - 1] == 0 and np.all(np.delete(out["rank"], [3, batch - 1]) == n)
    sn = np.linalg.svd(A, compute_uv=False)
    unit = out["sweeps"][:, None] * n * EPS
    assert np.all(np.abs(out["S"] - sn) <= (unit + (n + 8) * EPS) * np.maximum(sn[:, :1], 1e-300))
    USV = (out["U"] * out["S"][:, None, :]) @ out["V"].transpose(0, 2, 1)
    an = np.sqrt((A * A).sum(axis=(1, 2)))
    rec = np.sqrt(((A - USV) ** 2).sum(axis=(1, 2))) / np.where(an > 0, an, 1.0)
    assert np.all(rec <= unit[:, 0] + (n + 8) * EPS)
    ov = np.sqrt(((out["V"].transpose(0, 2, 1) @ out["V"] - np.eye(n)) ** 2).sum(axis=(1, 2)))
    ou = np.sqrt(((out["U"].transpose(0, 2, 1) @ out["U"] - np.eye(n)) ** 2).sum(axis=(1, 2)))
    assert np.all(ov <= 4 * unit[:, 0]) and np.all(ou <= 4 * unit[:, 0] + (n + 8) * EPS)
    for k in ("U", "S", "V", "rank", "sweeps"):
        assert np.array_equal(out[k][batch - 2], out[k][0])
    print(f"batched svd 16x8 x{batch}: sweeps {out['sweeps'].min()} to {out['sweeps'].max()}, worst reconstruction {rec.max() / EPS:.2f} eps")


@pytest.mark.parametrize("m,n", [(5, 3), (64, 32), (100, 33), (64, 64)])
def test_result_does_not_depend_on_the_batch_or_the_index(qr, plan, m, n):
    A7, _ = B.make_batch("mixed", m, n, batch=7)
    for src in (0, 1, 4):                                                      # Gaussian, rank-deficient, zero plus duplicated column
        A = A7.copy()
        A[5] = A7[src]
        o7, o1 = _svd(plan, A), _svd(plan, A[5:6])
        for k in ("U", "S", "V", "rank", "sweeps", "F", "tau", "jpvt"):
            assert np.array_equal(o7[k][5], o1[k][0]), (src, k)
            assert np.array_equal(o7[k][5], o7[k][src]), (src, k)


@pytest.mark.parametrize("m,n", [(5, 3), (64, 32), (100, 33), (256, 64)])
@pytest.mark.parametrize("e", [100, -100])
def test_scaling_by_a_power_of_two_is_exact(qr, plan, m, n, e):
    A, _ = B.make_batch("mixed", m, n)
    s = 2.0 ** e
    o, os_ = _svd(plan, A), _svd(plan, A * s)
    for k in ("U", "V", "sweeps", "rank", "info", "jpvt"):
        assert np.array_equal(o[k], os_[k]), k
    assert np.array_equal(os_["S"] / s, o["S"])


@pytest.mark.parametrize("m,n", [(33, 17), (100, 33)])
def test_padded_layout_is_respected_and_equals_the_packed_call(qr, plan, m, n):
    batch, tail, off = B.BATCH, 13, 1
    A, _ = B.make_batch("mixed", m, n)
    lda, ldu, ldv = m + 3, m + 1, n + 2                                       # odd leading dimensions
    sa, st, sj, ss, su, sv = lda * n + 5, n + 2, n + 3, n + 1, ldu * n + 3, ldv * n + 7
    view = lambda b, s, ld, cols, rows: np.lib.stride_tricks.as_strided(b[off:], (batch, cols, rows), (b.itemsize * s, b.itemsize * ld, b.itemsize))
    ref = _svd(plan, A)
    for ju, jv in (("U", "V"), ("N", "N")):
        bufs = {k: np.full(off + batch * s + tail, SENTINEL) for k, s in (("a", sa), ("t", st), ("s", ss), ("u", su), ("v", sv))}
        jbuf = np.full(off + batch * sj + tail, -9, dtype=np.int32)
        view(bufs["a"], sa, lda, n, m)[...] = A.transpose(0, 2, 1)
        d = {k: _up(v) for k, v in bufs.items()}
        dj, dinfo, drank, dsw = _up(jbuf), _ints(batch + 3), _ints(batch + 3), _ints(batch + 3)
        base = lambda t_: t_.data_ptr() + off * t_.element_size()              # bases one element off
        plan.gesvd_batched(ju, jv, base(d["a"]), m, n, lda, sa, base(dj), sj, base(d["t"]), st, base(d["s"]), ss, dinfo, batch,
                           dU=base(d["u"]) if ju == "U" else None, ldu=ldu, strideU=su, dV=base(d["v"]) if jv == "V" else None, ldv=ldv,
                           strideV=sv, drank=drank, dsweeps=dsw)
        plan.sync()
        h = {k: _down(v).copy() for k, v in d.items()}
        j2 = _down(dj).copy()
        assert np.array_equal(view(h["a"], sa, lda, n, m).transpose(0, 2, 1), ref["F"])
        assert np.array_equal(view(h["t"], st, n, 1, n)[:, 0, :], ref["tau"])
        assert np.array_equal(view(j2, sj, n, 1, n)[:, 0, :], ref["jpvt"])
        assert np.array_equal(view(h["s"], ss, n, 1, n)[:, 0, :], ref["S"])
        if ju == "U":
            assert np.array_equal(view(h["u"], su, ldu, n, m).transpose(0, 2, 1), ref["U"])
            view(h["u"], su, ldu, n, m)[...] = SENTINEL
        if jv == "V":
            assert np.array_equal(view(h["v"], sv, ldv, n, n).transpose(0, 2, 1), ref["V"])
            view(h["v"], sv, ldv, n, n)[...] = SENTINEL
        assert list(_down(drank)) == list(ref["rank"]) + [-9] * 3 and list(_down(dsw)) == list(ref["sweeps"]) + [-9] * 3
        assert list(_down(dinfo)) == [0] * batch + [-9] * 3
        view(h["a"], sa, lda, n, m)[...] = SENTINEL
        view(h["t"], st, n, 1, n)[...] = SENTINEL
        view(h["s"], ss, n, 1, n)[...] = SENTINEL
        view(j2, sj, n, 1, n)[...] = -9
        for k in h:                                                            # gaps, tails and unwanted outputs came back intact
            assert np.all(h[k] == SENTINEL), k
        assert np.all(j2 == -9)


def test_ormqr_still_works_on_the_factors_left_behind(qr, plan):
    m, n, batch = 33, 17, B.BATCH
    A, _ = B.make_batch("gaussian", m, n)
    out = _svd(plan, A)
    dQ = _up(np.zeros((batch, n, m)))
    plan.orgqr_batched(_up(_pack(out["F"])), m, n, m, m * n, _up(out["tau"]), n, dQ, m, m * n, batch)
    plan.sync()
    Q = _down(dQ).transpose(0, 2, 1)
    R = np.triu(out["F"][:, :n, :])
    AP = np.take_along_axis(A, out["jpvt"][:, None, :], axis=2)
    assert np.max(np.abs(AP - Q @ R)) <= (n + 8) * EPS * np.max(np.sqrt((A * A).sum(axis=(1, 2))))


def test_host_twin_and_python_wrapper_agree_with_the_device_call(qr, plan):
    for m, n in ((20, 6), (70, 40)):
        A, _ = B.make_batch("mixed", m, n)
        out = _svd(plan, A)
        U, S, V, rank = qr.svd_batched(A)
        assert U.shape == (B.BATCH, m, n) and S.shape == (B.BATCH, n) and V.shape == (B.BATCH, n, n) and rank.shape == (B.BATCH,)
        assert np.array_equal(U, out["U"]) and np.array_equal(S, out["S"]) and np.array_equal(V, out["V"])
        assert np.array_equal(rank, out["rank"])
        U0, S0, V0, rank0 = qr.svd_batched(A, compute_uv=False)
        assert U0 is None and V0 is None and np.array_equal(S0, S) and np.array_equal(rank0, rank)
        # the C entry point itself: U, V and rank optional, A untouched
        At = _pack(A)
        keep = At.copy()
        Sc = np.full((B.BATCH, n), SENTINEL)
        dp = C.POINTER(C.c_double)
        assert qr.lib.qr_svd_batched(At.ctypes.data_as(dp), m, n, B.BATCH, Sc.ctypes.data_as(dp), None, None, None) == 0
        assert np.array_equal(Sc, S) and np.array_equal(At, keep)
