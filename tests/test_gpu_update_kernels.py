"""-m gpu: the kernels of the row-append and signed-row updates (csrc/qr_update.hip) at the launch layer, one launch at a time, against
the plain extended-precision reference of the same operation (tests/hp_ref.py: tp_panel, tp_apply).

The plan-level tests (test_gpu_update.py, test_gpu_downdate.py) assert properties of R' and reach the kernels only with w = min(32, n - k),
ldt = 32 and a T the panel kernel wrote itself.  Here every wrapper (qrd_tp_* and qrd_th_*) is called directly:

  * buffers have odd leading dimensions, a base one double off, a sentinel column behind the matrix and sentinel or NaN padding rows
    (gpu_util.Buf); after every launch everything outside the documented output region must be bitwise what went in -- R's strict lower
    triangle, the rows >= w of C1, the columns >= w of R and T, the padding;
  * R', V and T (the panels) and C1, C2 (the applies) are compared separately, ||X - X_ld|| / ||X_ld|| against the longdouble instance on
    the same input, and bounded by max(4 x the float64 instance's error, eps) (gpu_util.within), capped at 50 kappa(R') eps for the
    panels and (w + p) eps for the applies;
  * the applies get V and T from the longdouble reference rounded to double, not from the panel kernel, with NaN below T's diagonal and
    in the rows p .. ld of V and C2: what the kernels promise not to read is poisoned;
  * the signed instance decides a sign per row (panel: t < p_add) and per lane and MFMA chain (apply: i + 4 q < p_add - l4): p_add runs
    over every value 0 .. 70 at p = 70 (all residues mod 16 and the 64-row wave boundary) and around the wave boundaries at p = 256;
  * the status word: a block whose column j* leaves d <= 0 gives col0 + j* + 1 and writes nothing; with the word already set th_panel,
    th_apply and th_colssq leave every buffer bitwise alone.

Unsigned inputs are those of test_gpu_update._inputs, signed ones those of test_gpu_downdate._inputs (the removed rows are rows of the
matrix R came from, so d > 0 with margin).  Every test prints its ratios (-s); a case that legitimately exceeds 4 x goes into MEASURED
with the ratio measured on an MI355X ("Accuracy against the extended-precision reference"), its bound is twice that ratio.
"""
import functools

import numpy as np
import pytest

import hp_ref as H
from gpu_util import Buf, bits, ivec, ivec_out, within
from test_gpu_downdate import _inputs as _signed_inputs
from test_gpu_update import SENTINEL, _inputs as _unsigned_inputs

pytestmark = pytest.mark.gpu

EPS = H.EPS
NAN = float("nan")
W_ALL = [1, 7, 31, 32]
P_ALL = [1, 15, 16, 17, 63, 64, 65, 255, 256]
APPLY_SHAPES = [(32, 256), (32, 17), (7, 65), (1, 1), (31, 100)]
NCOLS = [1, 31, 32, 33, 65]
LDTS = ("w", 33, 40)
SWEEP_P = 70
SWEEP_GROUPS = [range(a, min(a + 12, SWEEP_P + 1)) for a in range(0, SWEEP_P + 1, 12)]
P256_ADDS = [0, 63, 64, 65, 128, 192, 255, 256]

# tag -> the ratio to the float64 reference measured on an MI355X where it exceeds 4 (DESIGN.md has the table and the date); the bound
# of such a case is twice the ratio
MEASURED = {}


@pytest.fixture(scope="module")
def q(qr):
    qr.check(qr.lib.qrd_init(), "qrd_init")
    return qr


def _sync(q):
    q.check(q.lib.qrd_device_sync(), "sync")


def _f64(X):
    return np.asarray(X, dtype=np.float64)


def _err(X, Xld):
    d, n = H.norm(H.arr(X) - Xld), H.norm(Xld)
    return float(d / n) if n != 0 else float(d)


def _signed(w, p, p_add, nkeep=2 * 32):
    """(R, B) of test_gpu_downdate._inputs with nkeep rows of R's matrix kept, p - p_add of it removed and p_add new ones"""
    R, B, _, _ = _signed_inputs(w, p_add, p - p_add, nkeep + p_add)
    return R, B


@functools.lru_cache(maxsize=None)
def _panel_ref(kind, w, p, p_add=None, nkeep=64, zero_col=None):
    """the input and the two instances of the reference, computed once: (R, B, (R', V, T) in longdouble, (R', V, T) in float64)"""
    R, B = _unsigned_inputs(w, p) if kind == "u" else _signed(w, p, p_add, nkeep)
    R, B = R[:w, :w], B
    if zero_col is not None:
        B = B.copy()
        B[:, zero_col] = 0.0
        B.setflags(write=False)
    return R, B, H.tp_panel(R, B, p_add), H.tp_panel(R, B, p_add, np.float64)


def _launch_panel(q, R, B, p_add=None, ldt=33, col0=0, status=0):
    """qrd_tp_panel (p_add None) or qrd_th_panel on sentinel-framed buffers: (bR, bB, bT, status after)"""
    p, w = B.shape
    ldr, ldb = (w + 2) | 1, (p + 2) | 1
    bR = Buf(np.triu(R) + np.tril(np.full((w, w), SENTINEL), -1), ldr)
    bB = Buf(B, ldb, pad=NAN)
    bT = Buf(np.full((w, w), 11.5), ldt)
    if p_add is None:
        q.check(q.lib.qrd_tp_panel(None, bR.ptr, ldr, bB.ptr, ldb, p, w, bT.ptr, ldt), "qrd_tp_panel")
        _sync(q)
        return bR, bB, bT, 0
    st, sp = ivec([status])
    q.check(q.lib.qrd_th_panel(None, bR.ptr, ldr, bB.ptr, ldb, p, p_add, w, bT.ptr, ldt, col0, sp), "qrd_th_panel")
    _sync(q)
    return bR, bB, bT, int(ivec_out(st)[0])


def _panel_out(bR, bB, bT):
    """(R' with the caller's lower triangle, V, T) after the checks on everything the launch may not write"""
    w, p = bR.m, bB.m
    Rout = bR.check(np.triu(np.ones((w, w), bool)), "R")
    V = bB.check(np.ones((p, w), bool), "B")
    T = bT.check(np.ones((w, w), bool), "T")
    assert np.all(np.tril(T, -1) == 0.0), "T is upper triangular with zeros below its diagonal"
    return Rout, V, T


def _check_panel(tag, out, ld, f64):
    Rout, V, T = out
    cap = 50 * np.linalg.cond(_f64(ld[0])) * EPS
    for name, X, i in (("R'", np.triu(Rout), 0), ("V", V, 1), ("T", T, 2)):
        within(f"{tag} {name}", _err(X, ld[i]), _err(f64[i], ld[i]), cap, MEASURED)


@pytest.mark.parametrize("p", P_ALL)
@pytest.mark.parametrize("w", W_ALL)
def test_tp_panel_against_the_reference_and_th_panel_without_removed_rows(q, w, p):
    R, B, ld, f64 = _panel_ref("u", w, p)
    out = _panel_out(*_launch_panel(q, R, B)[:3])
    _check_panel(f"tp_panel w={w} p={p}", out, ld, f64)
    again = _panel_out(*_launch_panel(q, R, B, ldt=40)[:3])
    assert all(bits(a, b) for a, b in zip(out, again)), "a repeated launch (another ldt) is bitwise equal"
    *bufs, status = _launch_panel(q, R, B, p_add=p)
    assert status == 0
    signed = _panel_out(*bufs)
    assert all(bits(a, b) for a, b in zip(out, signed)), "th_panel with p_add = p is bitwise tp_panel"


def _check_signed_panel(q, w, p, p_add, nkeep=64):
    R, B, ld, f64 = _panel_ref("s", w, p, p_add, nkeep)
    *bufs, status = _launch_panel(q, R, B, p_add=p_add)
    assert status == 0
    out = _panel_out(*bufs)
    _check_panel(f"th_panel w={w} p={p} p_add={p_add}" + ("" if nkeep == 64 else f" nkeep={nkeep}"), out, ld, f64)
    *bufs, status = _launch_panel(q, R, B, p_add=p_add, col0=64)
    assert status == 0 and all(bits(a, b) for a, b in zip(out, _panel_out(*bufs))), "a repeated launch is bitwise equal"


@pytest.mark.parametrize("group", SWEEP_GROUPS, ids=lambda g: f"{g[0]}-{g[-1]}")
def test_th_panel_every_p_add_of_a_70_row_block(q, group):
    for p_add in group:
        _check_signed_panel(q, 32, SWEEP_P, p_add)


@pytest.mark.parametrize("p_add", P256_ADDS)
def test_th_panel_p_add_around_the_wave_boundaries_of_256_rows(q, p_add):
    _check_signed_panel(q, 32, 256, p_add)


def test_th_panel_hard_removal_256_of_296_rows(q):
    _check_signed_panel(q, 32, 256, 0, nkeep=40)


@pytest.mark.parametrize("w", [7, 32])
@pytest.mark.parametrize("kind,p,p_add", [("u", 65, None), ("s", 70, 37)])
def test_panel_zero_column_of_the_block(q, kind, p, p_add, w):
    """column 0 zero: tau_0 = 0, V(:, 0) = 0, row 0 of R untouched.  Column w - 1 zero on entry only: the reflectors to its left fill it in
    (as in LAPACK's dtpqrt), so it is compared with the reference like any other"""
    for j in sorted({0, w - 1}):
        R, B, ld, f64 = _panel_ref(kind, w, p, p_add, 64, j)
        *bufs, status = _launch_panel(q, R, B, p_add=p_add)
        assert status == 0
        out = _panel_out(*bufs)
        _check_panel(f"{'tp' if kind == 'u' else 'th'}_panel w={w} p={p} zero column {j}", out, ld, f64)
        if j == 0:
            Rout, V, T = out
            assert np.all(V[:, 0] == 0.0) and np.all(T[:, 0] == 0.0) and bits(np.triu(Rout)[0], R[0])


def _bad_block(w=32, p=70, p_add=37, jstar=5):
    """a signed block whose last removed row was never in R: zero but for 1000 in column j*, which no reflector to the left touches
    (its v entries are zero there), so that column j* finds d = alpha^2 + .. - 10^6 < 0"""
    R, B = _signed(w, p, p_add)
    B = B.copy()
    B[p - 1] = 0.0
    B[p - 1, jstar] = 1000.0
    for dt in (H.LD, np.float64):
        with pytest.raises(ArithmeticError) as ei:
            H.tp_panel(R, B, p_add, dt)
        assert ei.value.args[1] == jstar
    return R, B


@pytest.mark.parametrize("col0", [0, 64])
def test_th_panel_reports_the_failing_column_and_writes_nothing(q, col0):
    R, B = _bad_block()
    bR, bB, bT, status = _launch_panel(q, R, B, p_add=37, col0=col0)
    assert status == col0 + 5 + 1
    bR.check(None, "R")
    bB.check(None, "B")
    bT.check(None, "T")


def _launch_apply(q, V, T, C1, C2, ldt, trans=1, p_add=None, status=0):
    """qrd_tp_apply (p_add None) or qrd_th_apply with T's strict lower triangle and the padding rows of V and C2 holding NaN:
    (bC1, bC2, the read-only buffers, status after)"""
    p, w = V.shape
    ncols = C1.shape[1]
    ldt = w if ldt == "w" else ldt
    ldv, ldc1, ldc2 = (p + 2) | 1, (w + 2) | 1, (p + 4) | 1
    bV = Buf(V, ldv, pad=NAN)
    bT = Buf(np.triu(T) + np.tril(np.full((w, w), NAN), -1), ldt, pad=NAN)
    bC1, bC2 = Buf(C1, ldc1), Buf(C2, ldc2, pad=NAN)
    if p_add is None:
        q.check(q.lib.qrd_tp_apply(None, trans, bV.ptr, ldv, p, w, bT.ptr, ldt, bC1.ptr, ldc1, bC2.ptr, ldc2, ncols), "qrd_tp_apply")
        _sync(q)
        return bC1, bC2, (bV, bT), 0
    st, sp = ivec([status])
    q.check(q.lib.qrd_th_apply(None, bV.ptr, ldv, p, p_add, w, bT.ptr, ldt, bC1.ptr, ldc1, bC2.ptr, ldc2, ncols, sp), "qrd_th_apply")
    _sync(q)
    return bC1, bC2, (bV, bT), int(ivec_out(st)[0])


def _apply_out(bC1, bC2, ro, status=0):
    assert status == 0
    for b in ro:
        b.check(None, "V / T")
    return bC1.check(np.ones((bC1.m, bC1.n), bool), "C1"), bC2.check(np.ones((bC2.m, bC2.n), bool), "C2")


def _c12(w, p, ncols):
    rng = np.random.default_rng(31 * w + 7 * p + ncols)
    return rng.standard_normal((w, ncols)), rng.standard_normal((p, ncols))


def _check_apply(tag, out, V, T, C1, C2, p_add, trans):
    w, p = V.shape[1], V.shape[0]
    ld, f64 = H.tp_apply(V, T, C1, C2, p_add, trans), H.tp_apply(V, T, C1, C2, p_add, trans, np.float64)
    for name, i in (("C1", 0), ("C2", 1)):
        assert np.all(np.isfinite(out[i])), "NaN from below T's diagonal or from the padding rows"
        within(f"{tag} {name}", _err(out[i], ld[i]), _err(f64[i], ld[i]), (w + p) * EPS, MEASURED)


@pytest.mark.parametrize("ncols", NCOLS)
@pytest.mark.parametrize("w,p", APPLY_SHAPES)
def test_tp_apply_against_the_reference_and_th_apply_without_removed_rows(q, w, p, ncols):
    _, _, (_, Vld, Tld), _ = _panel_ref("u", w, p)
    V, T = _f64(Vld), _f64(Tld)
    C1, C2 = _c12(w, p, ncols)
    for trans in (0, 1):
        ldt = LDTS[(NCOLS.index(ncols) + trans) % 3]
        out = _apply_out(*_launch_apply(q, V, T, C1, C2, ldt, trans))
        _check_apply(f"tp_apply w={w} p={p} ncols={ncols} trans={trans} ldt={ldt}", out, V, T, C1, C2, None, trans)
        again = _apply_out(*_launch_apply(q, V, T, C1, C2, LDTS[(NCOLS.index(ncols) + trans + 1) % 3], trans))
        assert bits(out[0], again[0]) and bits(out[1], again[1]), "a repeated launch (another ldt) is bitwise equal"
    signed = _apply_out(*_launch_apply(q, V, T, C1, C2, ldt, p_add=p))
    assert bits(out[0], signed[0]) and bits(out[1], signed[1]), "th_apply with p_add = p is bitwise tp_apply(trans = 1)"


def _check_signed_apply(q, w, p, p_add, ncols):
    _, _, (_, Vld, Tld), _ = _panel_ref("s", w, p, p_add)
    V, T = _f64(Vld), _f64(Tld)
    C1, C2 = _c12(w, p, ncols)
    ldt = LDTS[p_add % 3]
    out = _apply_out(*_launch_apply(q, V, T, C1, C2, ldt, p_add=p_add))
    _check_apply(f"th_apply w={w} p={p} p_add={p_add} ncols={ncols} ldt={ldt}", out, V, T, C1, C2, p_add, 1)
    return out


@pytest.mark.parametrize("group", SWEEP_GROUPS, ids=lambda g: f"{g[0]}-{g[-1]}")
def test_th_apply_every_p_add_of_a_70_row_block(q, group):
    for p_add in group:
        _check_signed_apply(q, 32, SWEEP_P, p_add, 33)


@pytest.mark.parametrize("p_add", P256_ADDS)
def test_th_apply_p_add_around_the_wave_boundaries_of_256_rows(q, p_add):
    out = _check_signed_apply(q, 32, 256, p_add, 33)
    again = _check_signed_apply(q, 32, 256, p_add, 33)
    assert bits(out[0], again[0]) and bits(out[1], again[1])


def test_a_set_status_word_leaves_every_buffer_alone(q):
    """th_panel, th_apply and th_colssq return at once when the word is non-zero: nothing is written, the word keeps its value"""
    R, B, (_, Vld, Tld), _ = _panel_ref("s", 32, 70, 37)
    bR, bB, bT, status = _launch_panel(q, R, B, p_add=37, status=7)
    assert status == 7
    for b in (bR, bB, bT):
        b.check(None, "th_panel")
    C1, C2 = _c12(32, 70, 33)
    bC1, bC2, ro, status = _launch_apply(q, _f64(Vld), _f64(Tld), C1, C2, 33, p_add=37, status=7)
    assert status == 7
    for b in (bC1, bC2, *ro):
        b.check(None, "th_apply")
    bX, bacc = Buf(B[:, :3], 73, pad=NAN), Buf(np.array([[0.5, 1.5, 2.5]]).T, 3, extra=0)
    st, sp = ivec([7])
    q.check(q.lib.qrd_th_colssq(None, bX.ptr, 73, 70, 37, 3, bacc.ptr, sp), "qrd_th_colssq")
    _sync(q)
    assert ivec_out(st)[0] == 7
    bX.check(None, "X")
    bacc.check(None, "acc")


def test_shapes_outside_the_documented_range_are_refused(q):
    """-7 from the wrapper, which launches nothing: p = 0, p = 257, w = 33, a leading dimension below the row count"""
    b = Buf(np.zeros((8, 8)), 9)
    st, sp = ivec([0])
    a = b.ptr
    L = q.lib
    for p, w, ldb in ((0, 8, 9), (257, 8, 300), (8, 33, 9), (8, 8, 7)):
        assert L.qrd_tp_panel(None, a, 33, a, ldb, p, w, a, 33) == -7
        assert L.qrd_th_panel(None, a, 33, a, ldb, p, max(p, 0), w, a, 33, 0, sp) == -7
        assert L.qrd_tp_apply(None, 1, a, ldb, p, w, a, 33, a, 33, a, ldb, 4) == -7
        assert L.qrd_th_apply(None, a, ldb, p, max(p, 0), w, a, 33, a, 33, a, ldb, 4, sp) == -7
    assert L.qrd_th_panel(None, a, 9, a, 9, 8, 9, 8, a, 9, 0, sp) == -7            # p_add > p
    assert L.qrd_th_colssq(None, a, 300, 257, 0, 1, a, sp) == -7 and L.qrd_th_colssq(None, a, 7, 8, 0, 1, a, sp) == -7
    _sync(q)
    b.check(None, "a refused call")
    assert ivec_out(st)[0] == 0


def _ssq_ld(x):
    x = H.arr(x)
    return (x * x).sum()


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_tp_colssq_add(q, rows):
    rng = np.random.default_rng(rows)
    X, acc = rng.random((rows, 3)) - 0.5, np.array([0.75, 3.0, 1e-3])
    ldx = (rows + 2) | 1
    bX, bacc = Buf(X, ldx, pad=NAN), Buf(acc[:, None], 3, extra=0)
    q.check(q.lib.qrd_tp_colssq_add(None, bX.ptr, ldx, rows, 3, bacc.ptr), "qrd_tp_colssq_add")
    _sync(q)
    bX.check(None, "X")
    got = bacc.check(np.ones((3, 1), bool), "acc")[:, 0]
    for c in range(3):
        ref = H.arr(acc[c]) + _ssq_ld(X[:, c])
        e = abs(float((H.arr(got[c]) - ref) / ref))
        print(f"tp_colssq_add rows={rows} column {c}: {e / EPS:.2f} eps (bound {rows})")
        assert e <= rows * EPS


@pytest.mark.parametrize("p", [1, 255, 256])
def test_th_colssq_and_its_clamp_at_zero(q, p):
    """column 2's removed rows outweigh the accumulator and the added rows whenever there are any: exactly 0.0"""
    rng = np.random.default_rng(50 + p)
    clamped = 0
    for p_add in sorted({0, min(64, p), p}):
        X, acc = rng.random((p, 3)) - 0.5, np.array([40.0, 3.0 + p / 4.0, 1e-3])
        X[p_add:, 2] = 10.0 * (0.5 + rng.random(p - p_add))
        ldx = (p + 2) | 1
        bX, bacc = Buf(X, ldx, pad=NAN), Buf(acc[:, None], 3, extra=0)
        st, sp = ivec([0])
        q.check(q.lib.qrd_th_colssq(None, bX.ptr, ldx, p, p_add, 3, bacc.ptr, sp), "qrd_th_colssq")
        _sync(q)
        assert ivec_out(st)[0] == 0
        bX.check(None, "X")
        got = bacc.check(np.ones((3, 1), bool), "acc")[:, 0]
        for c in range(3):
            a, d = _ssq_ld(X[:p_add, c]), _ssq_ld(X[p_add:, c])
            ref, mass = H.arr(acc[c]) + a - d, float(H.arr(acc[c]) + a + d)
            if ref < -p * EPS * mass:
                assert bits(got[c], 0.0), (p, p_add, c, got[c])
                clamped += 1
            else:
                e = abs(float(H.arr(got[c]) - ref)) / mass
                print(f"th_colssq p={p} p_add={p_add} column {c}: {e / EPS:.2f} eps of the mass (bound {p})")
                assert got[c] >= 0.0 and e <= p * EPS
        assert (p_add == p) or bits(got[2], 0.0)
    assert clamped >= 1


@pytest.mark.parametrize("n", [1, 256, 257])
def test_tp_sqrt_is_bitwise_numpy(q, n):
    x = np.random.default_rng(n).random(n) * 1e3
    x[0] = 0.0 if n > 1 else 2.0
    bi, bo = Buf(x[:, None], n, extra=0), Buf(np.full((n, 1), -1.0), n, extra=0)
    q.check(q.lib.qrd_tp_sqrt(None, bi.ptr, bo.ptr, n), "qrd_tp_sqrt")
    _sync(q)
    bi.check(None, "in")
    assert bits(bo.check(np.ones((n, 1), bool), "out")[:, 0], np.sqrt(x))
