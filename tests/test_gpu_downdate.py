"""-m gpu: row removal (mi355x_qr.h section 6b) against numpy / LAPACK.

Data: standard-normal rows from a fixed seed; R is numpy's QR of all rows, the removed rows are a random subset of them, and the
reference is numpy's QR of the surviving rows (plus the new ones), sign-normalised.  qr_tphqrt_dev: the Gram identity
R'^T R' = R^T R + B^T S B to n eps of |R^T R|, R' against numpy to 50 kappa(R') eps, R's strict lower triangle untouched, bitwise-equal
repeats; p_del = 0 is bitwise qr_tpqrt_dev; the guard's refusals.  qr_tphmqrt_dev on [R ; B] itself and on random columns.  The
accumulator's pop / slide and qr_lstsq_rolling against numpy.linalg.lstsq to the bounds of test_gpu_update / test_gpu_lstsq.

CPU emulation of the kernels' arithmetic (blocked, panel width 32): pure removal 0.8 .. 2.0 eps (Gram) and 1.6 .. 17.8 eps (R', the
largest at kappa 86 with n + 8 surviving rows); mixed 1.0 .. 1.6 eps (Gram) and 1.6 .. 2.5 eps (R'); 32 slides of a 256-row window at
n = 64: 7.4 eps.
"""
import functools

import numpy as np
import pytest

from gpu_util import dev, host, rel, zeros
from test_gpu_lstsq import _check
from test_gpu_update import SENTINEL, TW, _gram_err, _strided, _unstrided

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _inputs(n, p_add, p_del, survivors):
    """(R of [kept ; removed] with the removed rows scattered among the kept ones, B = [new ; removed], kept, new); read-only"""
    rng = np.random.default_rng(7000 + 1000 * n + 10 * p_add + p_del + survivors)
    nkeep = survivors - p_add
    allrows = rng.standard_normal((nkeep + p_del, n))
    gone = np.sort(rng.choice(nkeep + p_del, p_del, replace=False))
    mask = np.ones(nkeep + p_del, bool)
    mask[gone] = False
    new = rng.standard_normal((p_add, n))
    R = np.triu(np.linalg.qr(allrows, mode="r"))
    out = (R, np.vstack([new, allrows[gone]]), allrows[mask], new)
    for a in out:
        a.setflags(write=False)
    return out


def _tphqrt(qr, plan, R, B, p_add, p_del, off=1):
    """qr_tphqrt_dev on odd leading dimensions and a base one double off.  Returns (dR contents with whatever lies below the diagonal,
    V, T, the device buffers)"""
    n, p = R.shape[0], B.shape[0]
    assert p == p_add + p_del
    ldr, ldb = (n + 2) | 1, (p + 2) | 1
    Rin = np.triu(R) + np.tril(np.full((n, n), SENTINEL), -1)
    tR, dR = _strided(Rin, ldr, off, -3.5)
    tB, dB = _strided(B, ldb, off, -3.5)
    dT = zeros(TW, n)
    plan.tphqrt(dR, n, ldr, dB, p_add, p_del, ldb, dT, TW)
    Rout, V = _unstrided(tR, n, n, ldr, off), _unstrided(tB, p, n, ldb, off)
    # nothing outside the two blocks is written
    assert np.all(tR.cpu().numpy()[off:].reshape(n, ldr)[:, n:] == -3.5) and np.all(tB.cpu().numpy()[off:].reshape(n, ldb)[:, p:] == -3.5)
    assert np.all(tR.cpu().numpy()[:off] == -3.5) and np.all(tB.cpu().numpy()[:off] == -3.5)
    return Rout, V, host(dT), (dR, ldr, dB, ldb, dT, (tR, tB))


def _check_update(qr, what, n, p_add, p_del, survivors):
    R, B, kept, new = _inputs(n, p_add, p_del, survivors)
    plan = qr.Plan(n, n, 0, 0)
    Rout, V, T, _ = _tphqrt(qr, plan, R, B, p_add, p_del)
    Rn = np.triu(Rout)
    G0 = R.T @ R
    g = np.linalg.norm(Rn.T @ Rn - (G0 + new.T @ new - B[p_add:].T @ B[p_add:])) / np.linalg.norm(G0)
    Rl = np.linalg.qr(np.vstack([kept, new]), mode="r")
    sg = np.sign(np.diag(Rl)) * np.sign(np.diag(Rn))
    kappa = np.linalg.cond(Rn)
    e = rel(Rn, sg[:, None] * Rl)
    print(f"{what} n={n} p_add={p_add} p_del={p_del} ({survivors} surviving rows): gram {g / EPS:.2f} eps (bound {n}), "
          f"R' vs numpy {e / EPS:.2f} eps at kappa {kappa:.1f} (bound {50 * kappa:.0f})")
    assert np.all(np.isfinite(Rout)) and np.all(np.isfinite(V))
    assert g <= n * EPS
    assert e <= 50 * kappa * EPS
    assert np.array_equal(np.tril(Rout, -1), np.tril(np.full((n, n), SENTINEL), -1)), "the strict lower triangle of dR is the caller's"
    for k in range(0, n, TW):                      # each panel's T block is upper triangular
        assert np.all(np.tril(T[:min(TW, n - k), k:k + TW], -1) == 0.0)
    R2, V2, T2, _ = _tphqrt(qr, plan, R, B, p_add, p_del)
    assert np.array_equal(Rout, R2) and np.array_equal(V, V2) and np.array_equal(T, T2)
    plan.close()


@pytest.mark.parametrize("n,p_del", [(32, 1), (33, 16), (96, 100), (160, 37), (200, 256), (64, 256)])
def test_pure_removal_gram_identity_numpy_lower_triangle_and_determinism(qr, n, p_del):
    _check_update(qr, "removal", n, 0, p_del, 2 * n)


@pytest.mark.parametrize("n,p_del", [(96, 100), (200, 256)])
def test_hard_removal_with_few_surviving_rows(qr, n, p_del):
    """n + 8 rows survive: the CPU emulation gives 8.9 eps at kappa 28 and 17.8 eps at kappa 86 against numpy"""
    _check_update(qr, "hard removal", n, 0, p_del, n + 8)


@pytest.mark.parametrize("n,p_add,p_del", [(33, 1, 1), (96, 60, 40), (200, 128, 128)])
def test_mixed_add_and_remove_in_one_pass(qr, n, p_add, p_del):
    _check_update(qr, "mixed", n, p_add, p_del, 2 * n)


def test_without_removed_rows_the_result_is_bitwise_tpqrt(qr):
    n, p = 96, 100
    R, B, _, _ = _inputs(n, p, 0, 2 * n + p)           # R of 2 n rows, then p more
    plan = qr.Plan(n, n, 0, 0)
    Rh, Vh, Th, _ = _tphqrt(qr, plan, R, B, p, 0)
    ldr, ldb = (n + 2) | 1, (p + 2) | 1
    tR, dR = _strided(np.triu(R) + np.tril(np.full((n, n), SENTINEL), -1), ldr, 1, -3.5)
    tB, dB = _strided(B, ldb, 1, -3.5)
    dT = zeros(TW, n)
    plan.tpqrt(dR, n, ldr, dB, p, ldb, dT, TW)
    plan.sync()
    assert np.array_equal(Rh, _unstrided(tR, n, n, ldr, 1)) and np.array_equal(Vh, _unstrided(tB, p, n, ldb, 1))
    assert np.array_equal(Th, host(dT))
    plan.close()


def test_an_exactly_zero_column_of_the_block_leaves_its_column_of_r_alone(qr):
    """column 0 of every added and removed row is zero (so it was zero in those rows of the matrix R came from): tau_0 = 0"""
    n, p_add, p_del = 96, 20, 30
    rng = np.random.default_rng(5)
    kept, old, new = rng.standard_normal((2 * n, n)), rng.standard_normal((p_del, n)), rng.standard_normal((p_add, n))
    old[:, 0] = 0.0
    new[:, 0] = 0.0
    R = np.triu(np.linalg.qr(np.vstack([kept, old]), mode="r"))
    B = np.vstack([new, old])
    plan = qr.Plan(n, n, 0, 0)
    Rout, V, T, _ = _tphqrt(qr, plan, R, B, p_add, p_del)
    Rn = np.triu(Rout)
    assert np.all(V[:, 0] == 0.0) and T[0, 0] == 0.0
    assert np.array_equal(Rn[:, 0], R[:, 0]) and np.array_equal(Rn[0], R[0])
    g = np.linalg.norm(Rn.T @ Rn - (R.T @ R + new.T @ new - old.T @ old)) / np.linalg.norm(R.T @ R)
    print(f"zero column: gram {g / EPS:.2f} eps (bound {n})")
    assert g <= n * EPS
    plan.close()


def test_apply_on_the_stacked_matrix_and_the_signed_norm(qr):
    n, p_add, p_del = 96, 60, 40
    p = p_add + p_del
    R, B, _, _ = _inputs(n, p_add, p_del, 2 * n)
    plan = qr.Plan(n, n, 0, 0)
    Rout, _, _, (dR, ldr, dV, ldv, dT, _keep) = _tphqrt(qr, plan, R, B, p_add, p_del)
    d1, d2 = dev(R), dev(B)
    plan.tphmqrt(dV, p_add, p_del, n, ldv, dT, TW, d1, n, d2, p, n)
    plan.sync()
    out = np.vstack([host(d1), host(d2)])
    want = np.vstack([np.triu(Rout), np.zeros((p, n))])
    err = np.linalg.norm(out - want) / np.linalg.norm(np.vstack([R, B]))
    print(f"Theta [R ; B] - [R' ; 0]: {err / EPS:.2f} eps of |[R ; B]| (bound {n})")
    assert err <= n * EPS
    S = np.where(np.arange(p) < p_add, 1.0, -1.0)
    rng = np.random.default_rng(n + p)
    for nrhs in (1, 17, 65):
        C1, C2 = rng.standard_normal((n, nrhs)), rng.standard_normal((p, nrhs))
        ld1, ld2 = (n + 4) | 1, (p + 4) | 1
        t1, e1 = _strided(C1, ld1, 1, -3.5)
        t2, e2 = _strided(C2, ld2, 1, -3.5)
        plan.tphmqrt(dV, p_add, p_del, n, ldv, dT, TW, e1, ld1, e2, ld2, nrhs)
        plan.sync()
        Y1, Y2 = _unstrided(t1, n, nrhs, ld1, 1), _unstrided(t2, p, nrhs, ld2, 1)
        before = np.sum(C1 * C1, axis=0) + np.sum(S[:, None] * C2 * C2, axis=0)
        after = np.sum(Y1 * Y1, axis=0) + np.sum(S[:, None] * Y2 * Y2, axis=0)
        scale = np.sum(C1 * C1, axis=0) + np.sum(C2 * C2, axis=0)
        nerr = np.max(np.abs(after - before) / scale)
        print(f"tphmqrt nrhs={nrhs}: signed column norms {nerr / EPS:.2f} eps (bound {n + p})")
        assert rel(Y1, C1) > 0.01, "the transformation is not the identity"
        assert nerr <= (n + p) * EPS
        for t, rows, ld in ((t1, n, ld1), (t2, p, ld2)):       # nothing outside the blocks is written
            raw = t.cpu().numpy()
            assert raw[0] == -3.5 and np.all(raw[1:].reshape(nrhs, ld)[:, rows:] == -3.5)
    plan.close()


@pytest.mark.parametrize("col", [0, 70])
def test_a_removal_that_leaves_no_positive_definite_triangle_is_refused(qr, col):
    """R = I and the row 2 e_col: d = 1 - 4 < 0 at that column (col = 70: in the third panel)"""
    n = 96
    plan = qr.Plan(n, n, 0, 0)
    B = np.zeros((1, n))
    B[0, col] = 2.0
    dR, dB, dT = dev(np.eye(n)), dev(B), zeros(TW, n)
    with pytest.raises(qr.QRError) as ei:
        plan.tphqrt(dR, n, n, dB, 0, 1, 1, dT, TW)
    assert ei.value.status == qr.QR_E_NOTPD and ei.value.info == col + 1
    # the plan is usable afterwards: the same call on a row that is in the matrix
    B[0, col] = 0.5
    dR, dB = dev(np.eye(n)), dev(B)
    plan.tphqrt(dR, n, n, dB, 0, 1, 1, dT, TW)
    Rn = np.triu(host(dR))
    assert abs(abs(Rn[col, col]) - np.sqrt(0.75)) <= 4 * EPS
    plan.close()


def _push(plan, acc, A, B):
    """push and drain: the chunk buffers are workspace of launches queued on the plan's stream, so they live until it has been drained"""
    dA, dB = dev(A), dev(B)
    acc.push(dA, A.shape[0], A.shape[0], dB, A.shape[0])
    plan.sync()


def _solve(plan, acc, n, nrhs):
    dX, dres = zeros(n, nrhs), zeros(nrhs, 1)
    acc.solve(dX, n, dres)
    plan.sync()
    return host(dX), host(dres)[:, 0]


def test_pop_of_a_row_that_was_never_pushed_leaves_the_accumulator_as_it_was(qr):
    n, nrhs, m = 48, 2, 192
    rng = np.random.default_rng(48)
    A, B = rng.standard_normal((m, n)), rng.standard_normal((m, nrhs))
    plan = qr.Plan(m, n, 0, 0)
    acc = qr.LsAccumulator(plan, n, nrhs)
    _push(plan, acc, A, B)
    R0, Z0 = acc.factor_host()
    X0, r0 = _solve(plan, acc, n, nrhs)
    with pytest.raises(qr.QRError) as ei:
        acc.pop(dev(3.0 * A[5:6]), 1, 1, dev(3.0 * B[5:6]), 1)
    assert ei.value.status == qr.QR_E_NOTPD
    R1, Z1 = acc.factor_host()
    X1, r1 = _solve(plan, acc, n, nrhs)
    assert acc.rows() == m
    assert np.array_equal(R0, R1) and np.array_equal(Z0, Z1) and np.array_equal(r0, r1) and np.array_equal(X0, X1)
    dA5, dB5 = dev(A[5:6]), dev(B[5:6])
    acc.pop(dA5, 1, 1, dB5, 1)                     # the row itself: legal
    assert acc.rows() == m - 1
    assert np.array_equal(host(dA5), A[5:6]) and np.array_equal(host(dB5), B[5:6]), "the inputs of a pop are untouched"
    X, r = _solve(plan, acc, n, nrhs)
    keep = np.delete(np.arange(m), 5)
    _check(A[keep], B[keep], X, r, np.linalg.cond(A[keep]))
    with pytest.raises(qr.QRError) as ei:          # more rows than are held
        acc.pop(zeros(m, n), m, m, zeros(m, nrhs), m)
    assert ei.value.status == qr.QR_E_ARG and acc.rows() == m - 1
    acc.close()
    plan.close()


def test_pop_in_two_blocks_matches_numpy_on_the_surviving_rows(qr):
    """n = 320: 300 rows leave in one call, which is two blocks (256 + 44) of the signed update"""
    n, nrhs, npop = 320, 2, 300
    m = 4 * n
    rng = np.random.default_rng(320)
    A, B = rng.standard_normal((m, n)), rng.standard_normal((m, nrhs))
    gone = np.sort(rng.choice(m, npop, replace=False))
    keep = np.setdiff1d(np.arange(m), gone)
    plan = qr.Plan(m, n, 0, 0)
    acc = qr.LsAccumulator(plan, n, nrhs)
    _push(plan, acc, A, B)
    acc.pop(dev(A[gone]), npop, npop, dev(B[gone]), npop)
    assert acc.rows() == m - npop
    X, r = _solve(plan, acc, n, nrhs)
    R, _ = acc.factor_host()
    G = A[keep].T @ A[keep]
    g = _gram_err(R, G)
    Xn = np.linalg.lstsq(A[keep], B[keep], rcond=None)[0]
    rn = np.linalg.norm(A[keep] @ Xn - B[keep], axis=0)
    print(f"pop {npop} of {m} rows at n={n}: X {rel(X, Xn) / EPS:.1f} eps, resid {np.max(np.abs(r - rn) / rn) / EPS:.1f} eps, "
          f"gram {g / EPS:.2f} eps (bound {n})")
    _check(A[keep], B[keep], X, r, np.linalg.cond(A[keep]))
    assert np.all(np.tril(R, -1) == 0.0)
    assert g <= n * EPS
    acc.close()
    plan.close()


def test_push_pop_push_equals_an_accumulator_that_saw_only_the_survivors(qr):
    n, nrhs = 48, 3
    rng = np.random.default_rng(4848)
    A, B = rng.standard_normal((4 * n + 40, n)), rng.standard_normal((4 * n + 40, nrhs))
    first, later = slice(0, 4 * n), slice(4 * n, 4 * n + 40)
    gone = np.sort(rng.choice(4 * n, n, replace=False))
    surv = np.concatenate([np.setdiff1d(np.arange(4 * n), gone), np.arange(4 * n, 4 * n + 40)])
    plan = qr.Plan(4 * n, n, 0, 0)
    acc = qr.LsAccumulator(plan, n, nrhs)
    _push(plan, acc, A[first], B[first])
    acc.pop(dev(A[gone]), n, n, dev(B[gone]), n)
    _push(plan, acc, A[later], B[later])
    assert acc.rows() == len(surv)
    X, r = _solve(plan, acc, n, nrhs)
    R, _ = acc.factor_host()
    ref = qr.LsAccumulator(plan, n, nrhs)
    _push(plan, ref, A[surv], B[surv])
    Xr, rr = _solve(plan, ref, n, nrhs)
    Rr, _ = ref.factor_host()
    kappa = np.linalg.cond(A[surv])
    g = _gram_err(R, A[surv].T @ A[surv])
    sg = np.sign(np.diag(R)) * np.sign(np.diag(Rr))
    print(f"push/pop/push vs survivors only: X {rel(X, Xr) / EPS:.1f} eps, R {rel(R, sg[:, None] * Rr) / EPS:.1f} eps at kappa {kappa:.1f}, "
          f"gram {g / EPS:.2f} eps (bound {n})")
    _check(A[surv], B[surv], X, r, kappa)
    _check(A[surv], B[surv], Xr, rr, kappa)
    assert g <= n * EPS
    assert rel(R, sg[:, None] * Rr) <= 50 * kappa * EPS
    ref.close()
    acc.close()
    plan.close()


def test_lstsq_rolling_matches_numpy_on_every_window(qr):
    m, n, nrhs, window, step = 640, 24, 2, 128, 32
    rng = np.random.default_rng(640)
    A, B = rng.standard_normal((m, n)), rng.standard_normal((m, nrhs))
    X, r = qr.lstsq_rolling(A, B, window, step)
    nwin = (m - window) // step + 1
    assert nwin == 17 and X.shape == (nwin, n, nrhs) and r.shape == (nwin, nrhs)
    worst, bmax = 0.0, 0.0
    for k in range(nwin):
        Aw, Bw = A[k * step:k * step + window], B[k * step:k * step + window]
        kappa = np.linalg.cond(Aw)
        Xn = np.linalg.lstsq(Aw, Bw, rcond=None)[0]
        rn = np.linalg.norm(Aw @ Xn - Bw, axis=0)
        bound = kappa + kappa ** 2 * np.linalg.norm(rn) / (np.linalg.norm(Aw, 2) * np.linalg.norm(Xn))
        worst, bmax = max(worst, rel(X[k], Xn) / (bound * EPS)), max(bmax, bound)
        assert rel(X[k], Xn) <= 50 * bound * EPS, k
        assert np.max(np.abs(r[k] - rn) / rn) <= 1e-12, k
    print(f"rolling {nwin} windows: worst X error {worst:.2f} of the perturbation bound (limit 50)")
    x1, r1 = qr.lstsq_rolling(A, B[:, 0], window, step)
    # one right-hand side alone: both results lie within 50 bound eps of numpy's, so within 100 of each other
    assert x1.shape == (nwin, n) and r1.shape == (nwin,) and rel(x1, X[:, :, 0]) <= 100 * bmax * EPS
    X2, r2 = qr.lstsq_rolling(A, B, window, step)
    assert np.array_equal(X, X2) and np.array_equal(r, r2)
    qr.release_cached_plans()


def test_gram_drift_after_32_slides(qr):
    """rounding adds at most linearly in the slides: 33 n eps for the push and 32 slides (the CPU emulation shows 7.4 eps)"""
    n, window, step, slides = 64, 256, 32, 32
    m = window + slides * step
    rng = np.random.default_rng(64256)
    A, B = rng.standard_normal((m, n)), rng.standard_normal((m, 1))
    plan = qr.Plan(window, n, 0, 0)
    acc = qr.LsAccumulator(plan, n, 1)
    _push(plan, acc, A[:window], B[:window])
    for k in range(1, slides + 1):
        o, e = (k - 1) * step, (k - 1) * step + window
        acc.slide(dev(A[e:e + step]), step, step, dev(B[e:e + step]), step, dev(A[o:o + step]), step, step, dev(B[o:o + step]), step)
    assert acc.rows() == window
    R, _ = acc.factor_host()
    Aw = A[m - window:]
    g = _gram_err(R, Aw.T @ Aw)
    print(f"gram drift after {slides} slides at n={n}: {g / EPS:.2f} eps (bound {33 * n})")
    assert g <= 33 * n * EPS
    X, r = _solve(plan, acc, n, 1)
    _check(Aw, B[m - window:], X, r, np.linalg.cond(Aw))
    acc.close()
    plan.close()
