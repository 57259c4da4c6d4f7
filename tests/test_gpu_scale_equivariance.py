"""-m gpu: bitwise scale equivariance of every factor and solve path.

For a power of two s, factoring s A must give BITWISE s R and the same V, tau, T, jpvt, ranks, status words and sweep counts, and
solving with a right-hand side scaled by an independent power of two t must give bitwise (t / s) X, as long as nothing leaves the
normal range and every decision taken on the device is homogeneous in the data.  No tolerance is involved: a kernel that fails holds
an absolute constant, a non-homogeneous shortcut or an over/underflow.  tests/test_hp_ref.py shows the property for a plain numpy
Householder QR at the same scales.

Scales: s in {2^40, 2^-40, 2^301, 2^-299} (odd exponents on purpose: the Gram rescale of the Householder panels rounds its exponent to
even), t in {1, 2^-77}.  Every square stays more than 400 binades inside the normal range.  Inputs are uniform in [-0.5, 0.5) from a
fixed seed (the ill-conditioned panels are the constructions of the tests whose entry they use); rank deficiency comes from sums of
columns with small-integer coefficients.  Each case runs once unscaled (cached) and once per scale; outputs are divided by the exact
power of two before `np.array_equal`.

The cases are the smallest shapes that reach each route; where a route is observable (guard and status words, Plan.route_stats(), the
fused batched route's shape rule) the case asserts it, so that it cannot silently take another one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import test_gpu_batched as tb
import test_gpu_batched_pivot as tbp
import test_gpu_panel_cqr as tcq
import test_gpu_panel_fused as tpf
from gpu_util import dev, host, zeros
from test_gpu_downdate import _tphqrt
from test_gpu_kernels import _cholqr_leaf
from test_gpu_svd import _gesvd, _gesvj
from test_gpu_update import TW, _tpqrt

pytestmark = pytest.mark.gpu

SCALES = [2.0 ** 40, 2.0 ** -40, 2.0 ** 301, 2.0 ** -299]
RHS_SCALES = [1.0, 2.0 ** -77]
_BASE = {}


def _exp(x):
    return f"2^{int(np.log2(x))}"


def U(seed, *shape):
    """uniform in [-0.5, 0.5), fixed seed"""
    return np.random.default_rng(seed).random(shape) - 0.5


def _rank_deficient(seed, m, n, r):
    """m x n of rank r: the trailing columns are sums of the leading r with coefficients in {-2 .. 2}"""
    rng = np.random.default_rng(seed)
    A = rng.random((m, n)) - 0.5
    A[:, r:] = A[:, :r] @ rng.integers(-2, 3, size=(r, n - r)).astype(np.float64)
    return A


def _ill(seed, mk, w, cond):
    rng = np.random.default_rng(seed)
    Uo, _ = np.linalg.qr(rng.standard_normal((mk, w)))
    W, _ = np.linalg.qr(rng.standard_normal((w, w)))
    return (Uo * np.logspace(0, -np.log10(cond), w)) @ W.T


def _split(F, s):
    """the factored array as scale-free pieces: the tails below the diagonal as they are, the triangle divided by s"""
    n = min(F.shape[-2:])
    return np.tril(F, -1), np.triu(F[..., :n, :]) / s


def _equivariant(key, run, *scales):
    """run(1, ...) once (cached under `key`), run(*scales) now; every output must be bitwise the same"""
    if key not in _BASE:
        _BASE[key] = run(*([1.0] * len(scales)))
    base, got = _BASE[key], run(*scales)
    assert base.keys() == got.keys()
    bad = []
    for k in base:
        a, b = np.asarray(base[k]), np.asarray(got[k])
        if a.shape != b.shape or not np.array_equal(a, b, equal_nan=True):
            note = ""
            if a.shape == b.shape and a.dtype.kind == "f" and a.size:
                with np.errstate(all="ignore"):
                    d = np.abs(a - b) / np.maximum(np.abs(a), np.finfo(float).tiny)
                note = f" ({int((a != b).sum())} of {a.size} entries, worst relative difference {np.nanmax(d):.2e})"
            bad.append(k + note)
    assert not bad, f"{key} at scales {[float(np.log2(x)) for x in scales]} (log2): not bitwise equivariant in {bad}"
    return base


@pytest.fixture(scope="module")
def q(qr):
    """the kernel-level entry points with the signatures the panel test modules give them"""
    tcq.q.__wrapped__(qr)
    tpf.q.__wrapped__(qr)
    L = qr.lib
    L.qrd_panel_cqr_retry.restype = C.c_int
    L.qrd_panel_cqr_retry.argtypes = L.qrd_panel_cqr_q.argtypes + [C.c_int]
    return qr


@pytest.fixture(scope="module")
def plan(qr):
    p = qr.Plan(64, 8, 0, 0)              # the batched calls take the plan's stream, not its shape
    yield p
    p.close()


# ---- guarded leaf panel (qrd_panel_cholqr): CholeskyQR2 accepted, and refused into the Householder TSQR ----------------------------
def _leaf_input(kind, mk):
    w = 32
    if kind == "accepted":
        return U(mk, mk, w)
    if kind == "dependent":
        P = U(mk + 1, mk, w)
        P[:, 9] = P[:, 2]
        return P
    return _ill(7, mk, w, 1e10)


@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("kind", ["accepted", "dependent", "cond1e10"])
@pytest.mark.parametrize("mk", [513, 514])
def test_guarded_leaf_panel(q, mk, kind, s):
    """513 rows is the smallest height test_panel_cholqr2_fast_path uses, but an odd height never reaches the guarded route: the entry
    sends a leaf whose rows cannot be read two at a time straight to the Householder TSQR and leaves the guard word alone (0 for all
    three inputs).  514 rows is the smallest height on the CholeskyQR2 route, where the guard accepts the first input and refuses the
    other two; the verdict must not depend on s."""
    P = _leaf_input(kind, mk)

    def run(s):
        out, tau, T, V, guard, _ = _cholqr_leaf(q, s * P)
        tails, R = _split(out, s)
        return {"tails": tails, "R": R, "tau": tau, "T": T, "V": V, "guard": guard}
    base = _equivariant(("leaf", mk, kind), run, s)
    assert base["guard"] == (0 if kind == "accepted" or mk % 2 else 1), "the case is on the other side of the guard"


# ---- one-launch panel (qrd_panel_fused) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("mk,wh", [(256, 32), (1000, 64), (640, 128)])
def test_one_launch_panel(q, mk, wh, s):
    P = U(mk + wh, mk, wh)
    ws = tpf.Ws(q)

    def run(s):
        out, V, T, tau, G, st = tpf.run_panel(q, ws, s * P)
        tails, R = _split(out, s)
        return {"tails": tails, "R": R, "V": V, "T": T, "tau": tau, "G": G, "status": st}
    base = _equivariant(("fused", mk, wh), run, s)
    assert base["status"][0] == 0 and base["status"][1] == 0, "a leaf left the CholeskyQR2 route or a wait timed out"


# ---- full-width CholeskyQR2 panel (qrd_panel_cqr), first attempt and preconditioned retry -------------------------------------------
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("mk,w", [(300, 128), (5000, 96)])
def test_full_width_panel_first_attempt(q, mk, w, s):
    P = U(mk + w, mk, w)

    def run(s):
        out, V, T, tau, st = tcq.run_panel(q, s * P, qbuf=True)
        tails, R = _split(out, s)
        return {"tails": tails, "R": R, "V": V, "T": T, "tau": tau, "status": st}
    base = _equivariant(("cqr", mk, w), run, s)
    assert base["status"][0] == 0, "the guard refused a well-conditioned panel"


def _cqr_then_retry(q, P):
    """qrd_panel_cqr_q, and, refused, qrd_panel_cqr_retry with the same arguments: (status of the first attempt, out, V, T, tau, status)"""
    mk, w = P.shape
    dA, dV, dQ = dev(P), dev(np.zeros((mk, w))), dev(np.full((mk, w), np.nan))
    dT, dtau = dev(np.full((w, w), np.nan)), zeros(w, 1)
    ws = torch.full((int(q.lib.qrd_panel_cqr_ws_doubles()),), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (None, dA.data_ptr(), mk, mk, w, dtau.data_ptr(), dT.data_ptr(), w, dV.data_ptr(), mk, ws.data_ptr(), status.data_ptr(),
            dQ.data_ptr(), mk, None, 0)
    assert q.lib.qrd_panel_cqr_q(*args) == 0
    q.check(q.lib.qrd_device_sync(), "sync")
    first = status.cpu().numpy().copy()
    assert first[0] == 1, "the first attempt accepted the panel: nothing to retry"
    assert np.array_equal(host(dA), P), "a refused panel must be left exactly as it was"
    assert q.lib.qrd_panel_cqr_retry(*args, 0) == 0
    q.check(q.lib.qrd_device_sync(), "sync")
    return first, host(dA), host(dV), host(dT), host(dtau)[:, 0], status.cpu().numpy()


@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_full_width_panel_refused_then_retried(q, s):
    """a cond 1e9 panel: refused by the first attempt, accepted by the preconditioned retry (shifted CholeskyQR3)"""
    P = _ill(11, 4096, 128, 1e9)

    def run(s):
        first, out, V, T, tau, st = _cqr_then_retry(q, s * P)
        tails, R = _split(out, s)
        return {"first": first, "tails": tails, "R": R, "V": V, "T": T, "tau": tau, "status": st[:1]}
    base = _equivariant("cqr_retry", run, s)
    assert base["first"][0] == 1 and base["status"][0] == 0, "refused, then accepted by the retry"


# ---- qr_geqrf_dev end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("nb,ib", [(0, 0), (32, 8)])
@pytest.mark.parametrize("m,n", [(600, 200), (1541, 300), (65, 63)])
def test_geqrf_end_to_end(qr, m, n, nb, ib, s):
    A = U(m * n, m, n)

    def run(s):
        p = qr.Plan(m, n, nb, ib)
        dA, dtau, dQ = dev(s * A), zeros(n, 1), zeros(m, n)
        p.geqrf(dA, m, n, m, dtau)
        pnb = p.nb
        dT = zeros(pnb, n)
        p.build_t(dA, m, n, m, dtau, dT, pnb)
        p.applyq(dA, m, n, m, dtau, dQ, n, m, True)
        p.sync()
        tails, R = _split(host(dA), s)
        stats = p.route_stats()
        p.close()
        return {"tails": tails, "R": R, "tau": host(dtau)[:, 0], "T": host(dT), "Q": host(dQ),
                "routes": np.array([stats[k] for k in sorted(stats)])}
    _equivariant(("geqrf", m, n, nb, ib), run, s)


# ---- mmqr + explicitQR (host entry) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("kind", ["full", "zero_and_duplicate"])
def test_mmqr_and_explicit_qr(qr, kind, s):
    A = U(4, 200, 40)
    if kind != "full":
        A[:, 7] = 0.0
        A[:, 20] = A[:, 3]

    def run(s):
        F, tau = qr.mmqr(s * A)
        Q, R = qr.explicit_qr(F, tau)
        tails, Rf = _split(F, s)
        return {"tails": tails, "Rf": Rf, "tau": tau, "Q": Q, "R": R / s}
    base = _equivariant(("mmqr", kind), run, s)
    assert kind == "full" or base["tau"][7] == 0.0


# ---- section 3: ormqr, solve_r, gels -------------------------------------------------------------------------------------------------
def _factor_host(qr, A):
    """(F, tau) of the unscaled matrix, once"""
    key = ("factors", A.shape, float(A[0, 0]))
    if key not in _BASE:
        m, n = A.shape
        p = qr.Plan(m, n, 0, 0)
        dA, dtau = dev(A), zeros(n, 1)
        p.geqrf(dA, m, n, m, dtau)
        p.sync()
        _BASE[key] = (host(dA), host(dtau)[:, 0].copy())
        p.close()
    return _BASE[key]


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", [2.0 ** 301, 2.0 ** -299], ids=_exp)
@pytest.mark.parametrize("m,n", [(1000, 37), (200, 200)])
def test_ormqr(qr, m, n, s, t):
    """the factors are those of A with the triangle scaled by s (ormqr reads the tails and tau only); C is scaled by t"""
    F, tau = _factor_host(qr, U(m + n, m, n))

    def run(s, t):
        p = qr.Plan(m, n, 0, 0)
        nb = p.nb
        dA, dtau = dev(np.tril(F, -1) + s * np.triu(F)), dev(tau[:, None])
        dT = zeros(nb, n)
        p.build_t(dA, m, n, m, dtau, dT, nb)
        out = {}
        for nrhs in (1, 4, 5):
            Cm = U(nrhs, m, nrhs)
            for T, ldt in ((None, 0), (dT, nb)):
                Y = dev(t * Cm)
                p.ormqr("T", dA, m, n, m, dtau, Y, nrhs, m, dT=T, ldt=ldt)
                p.sync()
                out[f"QtC nrhs {nrhs} T {T is not None}"] = host(Y) / t
                p.ormqr("N", dA, m, n, m, dtau, Y, nrhs, m, dT=T, ldt=ldt)
                p.sync()
                out[f"QQtC nrhs {nrhs} T {T is not None}"] = host(Y) / t
        p.close()
        return out
    _equivariant(("ormqr", m, n), run, s, t)


def _trsm_case(qr, which, s, t):
    n = 129
    F, _ = _factor_host(qr, U(n, n, n))

    def run(s, t):
        p = qr.Plan(n, n, 0, 0)
        dA = dev(np.tril(F, -1) + s * np.triu(F))
        out = {}
        for nrhs in (3, 65):
            X = dev(t * U(nrhs, n, nrhs))
            getattr(p, which)(dA, n, n, X, nrhs, n)
            p.sync()
            out[f"X nrhs {nrhs}"] = host(X) * (s / t)
        p.close()
        return out
    _equivariant((which, n), run, s, t)


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_solve_r(qr, s, t):
    _trsm_case(qr, "solve_r", s, t)


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("m,n", [(1000, 37), (200, 200)])
def test_gels(qr, m, n, s, t):
    A, B = U(m + n + 1, m, n), U(m + n + 2, m, 3)

    def run(s, t):
        p = qr.Plan(m, n, 0, 0)
        dA, dtau, dB = dev(s * A), zeros(n, 1), dev(t * B)
        p.gels(dA, m, n, m, dtau, dB, 3, m)
        p.sync()
        tails, R = _split(host(dA), s)
        Y = host(dB)
        p.close()
        return {"tails": tails, "R": R, "tau": host(dtau)[:, 0], "X": Y[:n] * (s / t), "QtB tail": Y[n:] / t}
    _equivariant(("gels", m, n), run, s, t)


# ---- section 4: geqp3, rank, gelsp ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("rank", [70, 20])
def test_geqp3_rank_gelsp(qr, rank, s, t):
    m, n = 300, 70
    A = U(370, m, n) if rank == n else _rank_deficient(371, m, n, rank)
    B = U(372, m, 3)

    def run(s, t):
        p = qr.Plan(m, n, 0, 0)
        dA, dtau, dj = dev(s * A), zeros(n, 1), torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p.geqp3(dA, m, n, m, dj, dtau)
        r = p.rank(dA, m, n, m)
        p.sync()
        tails, R = _split(host(dA), s)
        out = {"tails": tails, "R": R, "tau": host(dtau)[:, 0], "jpvt": dj.cpu().numpy(), "rank": r}
        dA2, dB, dres = dev(s * A), dev(t * B), zeros(3, 1)
        r2 = p.gelsp(dA2, m, n, m, dj, dtau, dB, 3, m, dresid=dres)
        p.sync()
        out.update({"gelsp rank": r2, "gelsp jpvt": dj.cpu().numpy(), "X": host(dB)[:n] * (s / t), "resid": host(dres)[:, 0] / t})
        p.close()
        return out
    base = _equivariant(("geqp3", rank), run, s, t)
    assert base["rank"] == rank and base["gelsp rank"] == rank


# ---- section 5: solve_rt, gels_t, gels_wide ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_solve_rt(qr, s, t):
    _trsm_case(qr, "solve_rt", s, t)


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_gels_t_and_gels_wide(qr, s, t):
    m, n = 300, 70                                  # the tall matrix whose transpose is solved; the wide one is its transpose
    A, B = U(5300, m, n), U(5301, n, 3)

    def run(s, t):
        p = qr.Plan(m, n, 0, 0)
        Bp = np.zeros((m, 3))
        Bp[:n] = t * B
        dA, dtau, dB = dev(s * A), zeros(n, 1), dev(Bp)
        p.gels_t(dA, m, n, m, dtau, dB, 3, m)
        p.sync()
        tails, R = _split(host(dA), s)
        out = {"tails": tails, "R": R, "tau": host(dtau)[:, 0], "X gels_t": host(dB) * (s / t)}
        dW, dF, dtau2, dB2 = dev(s * A.T), zeros(m, n), zeros(n, 1), dev(Bp)
        p.gels_wide(dW, n, m, n, dF, m, dtau2, dB2, 3, m)
        p.sync()
        tails2, R2 = _split(host(dF), s)
        out.update({"wide tails": tails2, "wide R": R2, "wide tau": host(dtau2)[:, 0], "X gels_wide": host(dB2) * (s / t),
                    "wide A untouched": host(dW) / s})
        p.close()
        return out
    _equivariant("minnorm", run, s, t)


# ---- sections 6 / 6b: row append, signed-row update, the accumulator -----------------------------------------------------------------
def _update_inputs(n, p):
    rng = np.random.default_rng(6000 + 10 * n + p)
    X = rng.random((2 * n + p, n)) - 0.5             # R is that of all the rows: the last p_del of them can be removed again
    R = np.triu(np.linalg.qr(X, mode="r"))
    return X, R, rng.random((p, n)) - 0.5, rng.random((n, 4)) - 0.5, rng.random((p, 4)) - 0.5


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("n,p", [(33, 7), (96, 100)])
def test_tpqrt_and_tpmqrt(qr, n, p, s, t):
    _, R, B, C1, C2 = _update_inputs(n, p)

    def run(s, t):
        plan = qr.Plan(n, n, 0, 0)
        Rout, V, Ts, (dR, ldr, dV, ldv, dTs) = _tpqrt(qr, plan, s * R, s * B)
        out = {"R'": np.triu(Rout) / s, "V": V, "T": Ts[0]}
        d1, d2 = dev(t * C1), dev(t * C2)
        for trans in "TN":
            plan.tpmqrt(trans, dV, p, n, ldv, dTs[0], TW, d1, n, d2, p, 4)
            plan.sync()
            out["C1 " + trans], out["C2 " + trans] = host(d1) / t, host(d2) / t
        plan.close()
        return out
    _equivariant(("tpqrt", n, p), run, s, t)


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("n,p_add,p_del", [(33, 4, 3), (96, 60, 40)])
def test_tphqrt_and_tphmqrt(qr, n, p_add, p_del, s, t):
    p = p_add + p_del
    X, R, B, C1, C2 = _update_inputs(n, p)
    B = np.vstack([B[:p_add], X[-p_del:]])           # new rows, then rows that are in R

    def run(s, t):
        plan = qr.Plan(n, n, 0, 0)
        Rout, V, T, (dR, ldr, dV, ldv, dT, _keep) = _tphqrt(qr, plan, s * R, s * B, p_add, p_del)
        d1, d2 = dev(t * C1), dev(t * C2)
        plan.tphmqrt(dV, p_add, p_del, n, ldv, dT, TW, d1, n, d2, p, 4)
        plan.sync()
        plan.close()
        return {"R'": np.triu(Rout) / s, "V": V, "T": T, "C1": host(d1) / t, "C2": host(d2) / t}
    _equivariant(("tphqrt", n, p_add, p_del), run, s, t)


@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_refused_removal_reports_the_same_column(qr, s):
    """removing a row that was never added (three times a row that was): QR_E_NOTPD and the failing column at every scale"""
    n = 70
    X, R, _, _, _ = _update_inputs(n, 1)
    B = 3.0 * X[5:6]

    def run(s):
        plan = qr.Plan(n, n, 0, 0)
        with pytest.raises(qr.QRError) as ei:
            _tphqrt(qr, plan, s * R, s * B, 0, 1)
        plan.close()
        return {"status": ei.value.status, "info": ei.value.info}
    base = _equivariant("notpd", run, s)
    assert base["status"] == qr.QR_E_NOTPD and 1 <= base["info"] <= n


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_ls_accumulator_push_pop_slide_solve(qr, s, t):
    n, nrhs, m = 33, 2, 120
    A, B = U(633, m, n), U(634, m, nrhs)

    def run(s, t):
        plan = qr.Plan(m, n, 0, 0)
        acc = qr.LsAccumulator(plan, n, nrhs)
        out = {}

        def state(tag):
            R, Z = acc.factor_host()
            dX, dres = zeros(n, nrhs), zeros(nrhs, 1)
            acc.solve(dX, n, dres)
            plan.sync()
            out.update({tag + " R": np.triu(R) / s, tag + " Z": Z / t, tag + " X": host(dX) * (s / t), tag + " resid": host(dres)[:, 0] / t,
                        tag + " rows": acc.rows()})
        keep = []                                    # chunk buffers are workspace of queued launches: alive until the stream is drained
        for r0, r1 in ((0, 80), (80, 87)):
            keep.append((dev(s * A[r0:r1]), dev(t * B[r0:r1])))
            acc.push(keep[-1][0], r1 - r0, r1 - r0, keep[-1][1], r1 - r0)
            plan.sync()
        state("pushed")
        keep.append((dev(s * A[10:17]), dev(t * B[10:17])))
        acc.pop(keep[-1][0], 7, 7, keep[-1][1], 7)
        state("popped")
        keep.append((dev(s * A[87:120]), dev(t * B[87:120]), dev(s * A[40:60]), dev(t * B[40:60])))
        acc.slide(keep[-1][0], 33, 33, keep[-1][1], 33, keep[-1][2], 20, 20, keep[-1][3], 20)
        state("slid")
        acc.close()
        plan.close()
        return out
    _equivariant("lsacc", run, s, t)


# ---- section 7: Jacobi SVD -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("n", [33, 96])
def test_gesvj(qr, n, s):
    G = U(700 + n, n, n)

    def run(s):
        plan = qr.Plan(n, n, 0, 0)
        Uv, S, V, sw = _gesvj(plan, s * G)
        U0, S0, _, sw0 = _gesvj(plan, s * G, jobv="N")
        plan.close()
        return {"U": Uv, "S": S / s, "V": V, "sweeps": sw, "U values-only": U0, "S values-only": S0 / s, "sweeps values-only": sw0}
    _equivariant(("gesvj", n), run, s)


@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_gesvd_and_cond(qr, s):
    m, n = 300, 96
    A = U(7300, m, n)

    def run(s):
        Uv, S, V, sw, R = _gesvd(qr, s * A)
        _, S0, _, sw0, _ = _gesvd(qr, s * A, jobs="NN")
        plan = qr.Plan(m, n, 0, 0)
        c = plan.cond(dev(s * A), m, n, m, zeros(n, 1))
        plan.close()
        return {"U": Uv, "S": S / s, "V": V, "sweeps": sw, "R": R / s, "S values-only": S0 / s, "sweeps values-only": sw0, "cond": c}
    _equivariant("gesvd", run, s)


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
def test_gelss_rank_deficient(qr, s, t):
    m, n, r = 64, 40, 25
    A, B = _rank_deficient(764, m, n, r), U(765, m, 3)

    def run(s, t):
        plan = qr.Plan(m, n, 0, 0)
        dA, dB, dS = dev(s * A), dev(t * B), zeros(n, 1)
        rank = plan.gelss(dA, m, n, m, zeros(n, 1), dB, 3, m, dS)
        plan.sync()
        plan.close()
        return {"rank": rank, "S": host(dS)[:, 0] / s, "X": host(dB)[:n] * (s / t)}
    base = _equivariant("gelss", run, s, t)
    assert base["rank"] == r


# ---- sections 8 / 8b: batched --------------------------------------------------------------------------------------------------------
BATCHED = [(17, 17), (64, 32), (100, 33), (256, 64)]          # wave route, wave route at its edge, workgroup route, its LDS edge


def _batch(m, n):
    """three matrices; the middle one has rank n - 2 (n > 2)"""
    A = U(8000 + m + n, 3, m, n)
    A[1] = _rank_deficient(8001 + m, m, n, max(1, n - 2))
    return A


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("m,n", BATCHED)
def test_batched_unpivoted(qr, plan, m, n, s, t):
    A = U(8100 + m + n, 3, m, n)
    nrhs = 2
    Bm = U(8200 + m, 3, m, nrhs)
    fused = n + nrhs <= 64 and m <= qr.batched_max_rows(n + nrhs)
    assert fused == ((m, n) != (256, 64)), "the fused gels route is taken by every shape but the last"

    def run(s, t):
        F, tau, Q = tb._factor(plan, s * A)
        tails, R = _split(F, s)
        X, rss, info = tb._gels(plan, s * A, t * Bm)
        return {"tails": tails, "R": R, "tau": tau, "Q": Q, "X": X * (s / t), "rss": rss / t / t, "info": info}
    base = _equivariant(("batched", m, n), run, s, t)
    assert not base["info"].any()


@pytest.mark.parametrize("t", RHS_SCALES, ids=_exp)
@pytest.mark.parametrize("s", SCALES, ids=_exp)
@pytest.mark.parametrize("m,n", BATCHED)
def test_batched_pivoted(qr, plan, m, n, s, t):
    A = _batch(m, n)
    Bm = U(8300 + m, 3, m, 2)

    def run(s, t):
        F, tau, jp, Q = tbp._geqp3(plan, s * A)
        tails, R = _split(F, s)
        dF, drank = tbp._up(tbp._pack(F)), tbp._ints(3)
        plan.rank_batched(dF, m, n, m, m * n, drank, 3)
        plan.sync()
        out = {"tails": tails, "R": R, "tau": tau, "jpvt": jp, "Q": Q, "rank_batched": tbp._down(drank)}
        for minnorm in (True, False):
            X, resid, rank, jp2, _, _, tail = tbp._solve(plan, s * A, t * Bm, minnorm)
            tag = "gelsy " if minnorm else "gelsp "
            out.update({tag + "X": X * (s / t), tag + "resid": resid / t, tag + "rank": rank, tag + "jpvt": jp2, tag + "QtB tail": tail / t})
        return out
    base = _equivariant(("batched pivoted", m, n), run, s, t)
    want = np.array([n, max(1, n - 2), n])
    assert np.array_equal(base["rank_batched"], want) and np.array_equal(base["gelsy rank"], want) and np.array_equal(base["gelsp rank"], want)
