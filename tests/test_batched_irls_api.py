"""CPU-side checks of the batched robust and weighted least squares (mi355x_qr.h section 8j): declared, exported, bound, wired into the
build, the row limit against its byte formula, and every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batched_irls_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IRLS_API = ("qr_irls_batched_max_rows", "qr_irls_batched_dev", "qr_gels_weighted_batched_dev", "qr_lstsq_robust_batched")
NAN, INF = float("nan"), float("inf")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(IRLS_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(IRLS_API) <= exported
    for name in IRLS_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8j. Batched robust and weighted least squares" in txt
    assert txt.index("8j. Batched robust and weighted") > txt.index("8i. Batched bound-constrained")
    for name, value in (("QR_LOSS_LS", 0), ("QR_LOSS_HUBER", 1), ("QR_LOSS_BISQUARE", 2)):
        assert f"#define {name} {value}" in txt and getattr(qr, name) == value
        assert txt.index(f"#define {name} ") > txt.index("8j. Batched robust and weighted")
    assert callable(qr.Plan.irls_batched) and callable(qr.irls_batched_max_rows) and callable(qr.lstsq_robust_batched)
    assert callable(qr.lstsq_weighted_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_ir_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_irls_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_irls_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_irls.c" in mk and "qr_batched_irls" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_ir_args", "qrd_ir_solve", "qrd_ir_max_rows", "qrd_ir_wave_route"):
        assert w in dev


def test_max_rows_at_its_edges_and_against_its_byte_formula(qr):
    mr = qr.irls_batched_max_rows
    assert mr(0) == 0 and mr(-1) == 0 and mr(64) == 0 and mr(65) == 0
    assert mr(1) == 512 and mr(8) == 512 and mr(31) == 512
    assert mr(63) == R.MAX_ROWS_63 and mr(63) >= 256          # the shapes of the tests and the measurement fit

    # the budget: (n + 1) qb_ld(m) + 3 m + 2 n + 72 doubles within 160 KiB, qb_ld(x) the smallest value >= x that is 2 mod 32
    def ld(x):
        return ((x + 29) // 32) * 32 + 2

    def nbytes(m, n):
        return 8 * ((n + 1) * ld(m) + 3 * m + 2 * n + 72)

    for n in range(1, 64):
        m = mr(n)
        assert m == R.max_rows(n)
        assert n <= m <= 512
        assert nbytes(m, n) <= 160 * 1024
        assert m == 512 or nbytes(m + 1, n) > 160 * 1024
    assert any(mr(n) < 512 for n in range(32, 64))
    assert bool(qr.lib.qrd_ir_wave_route(64, 31)) and not qr.lib.qrd_ir_wave_route(65, 31) and not qr.lib.qrd_ir_wave_route(40, 32)
    assert bool(qr.lib.qrd_ir_wave_route(1, 1))


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h).  Every call below must reject its arguments before it reaches a
    device, or have batch == 0."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


def test_device_call_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    def call(plan=P, loss=1, tune=0.0, A=d, m=20, n=8, lda=20, sa=160, B=d, sb=20, pr=d, spr=20, sc=d, X0=d, sx0=8, tol=1e-8, maxit=0, X=d, sx=8,
             W=d, sw=20, so=d, res=d, it=di, st=di, info=di, batch=3):
        return L.qr_irls_batched_dev(plan, loss, tune, A, m, n, lda, sa, B, sb, pr, spr, sc, X0, sx0, tol, maxit, X, sx, W, sw, so, res, it, st,
                                     info, batch)

    def shaped(m, n, **kw):
        return call(m=m, n=n, lda=m, sa=m * n, sb=m, spr=m, sx0=n, sx=n, sw=m, **kw)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(A=None) == E and call(B=None) == E and call(X=None) == E and call(info=None) == E
    assert call(pr=None, batch=0) == 0 and call(sc=None, batch=0) == 0 and call(X0=None, sx0=0, batch=0) == 0            # the optional inputs
    assert call(W=None, sw=0, batch=0) == 0 and call(so=None, res=None, it=None, st=None, batch=0) == 0                   # and outputs
    assert call(loss=-1) == E and call(loss=3) == E and all(call(loss=k, batch=0) == 0 for k in (0, 1, 2))
    assert call(tune=NAN) == E and call(tune=INF) == E and call(tune=-INF) == E
    assert call(tune=-1.0, batch=0) == 0 and call(tune=2.5, batch=0) == 0
    assert call(tol=-1e-300) == E and call(tol=NAN) == E and call(tol=0.0, batch=0) == 0 and call(tol=0.5, batch=0) == 0
    assert call(n=0) == E and call(n=-1) == E and shaped(70, 64) == E and shaped(70, 65) == E and shaped(70, 63, batch=0) == 0
    assert shaped(7, 8) == E and shaped(8, 8, batch=0) == 0 and shaped(1, 1, batch=0) == 0                               # m < n
    mr = L.qr_irls_batched_max_rows(63)
    assert 0 < mr < 512 and shaped(mr, 63, batch=0) == 0 and shaped(mr + 1, 63) == E                                     # m above the rows held
    assert shaped(512, 8, batch=0) == 0 and shaped(513, 8) == E
    assert call(lda=19) == E and call(sa=159) == E and call(lda=21, sa=167) == E and call(lda=21, sa=168, batch=0) == 0
    assert call(sb=19) == E and call(sx=7) == E and call(sw=19) == E and call(sx0=7) == E
    assert call(spr=19) == E and call(spr=1) == E and call(spr=-1) == E and call(spr=0, batch=0) == 0 and call(spr=21, batch=0) == 0
    assert call(pr=None, spr=19) == E and call(pr=None, spr=0, batch=0) == 0                                             # checked without weights too
    assert call(maxit=-5, batch=0) == 0 and call(maxit=1, batch=0) == 0
    assert call(batch=-1) == E
    assert call(batch=0, A=None) == E and call(batch=0, sx=7) == E and call(batch=0, spr=3) == E and call(batch=0, loss=7) == E   # the checks come first
    assert list(ibuf) == [0, 0, 0, 0]

    def wls(plan=P, A=d, m=20, n=8, lda=20, sa=160, B=d, sb=20, pr=d, spr=20, X=d, sx=8, res=d, info=di, batch=3):
        return L.qr_gels_weighted_batched_dev(plan, A, m, n, lda, sa, B, sb, pr, spr, X, sx, res, info, batch)

    assert wls(batch=0) == 0 and wls(pr=None, res=None, batch=0) == 0
    assert wls(plan=None) == E and wls(A=None) == E and wls(B=None) == E and wls(X=None) == E and wls(info=None) == E
    assert wls(m=7) == E and wls(lda=19) == E and wls(sa=159) == E and wls(sb=19) == E and wls(spr=19) == E and wls(sx=7) == E and wls(batch=-1) == E
    assert list(ibuf) == [0, 0, 0, 0]


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p_ = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p_, m=5, n=3, b=p_, loss=1, tune=0.0, pr=p_, sc=p_, x0=p_, tol=1e-8, maxit=0, batch=2, X=p_, W=p_, so=p_, res=p_, it=inf, st=inf,
             info=inf):
        return L.qr_lstsq_robust_batched(A, m, n, b, loss, tune, pr, sc, x0, tol, maxit, batch, X, W, so, res, it, st, info)

    assert twin(batch=0) == 0 and twin(batch=0, pr=None, sc=None, x0=None, W=None, so=None, res=None, it=None, st=None) == 0
    assert twin(A=None) == E and twin(b=None) == E and twin(X=None) == E and twin(info=None) == E
    assert twin(m=2) == E and twin(n=0) == E and twin(m=70, n=64) == E and twin(batch=-1) == E
    assert twin(loss=3) == E and twin(loss=-1) == E and twin(tune=NAN) == E and twin(tune=INF) == E and twin(tol=-1.0) == E and twin(tol=NAN) == E
    assert twin(m=513, batch=0) == E and twin(m=512, batch=0) == 0 and twin(batch=0, A=None) == E
    assert list(inf) == [0] * 16


def test_python_wrappers_raise_on_bad_shapes(qr):
    z = np.zeros
    bad = [
        lambda: qr.lstsq_robust_batched(z((6, 4)), z((3, 6))),                             # A 2-D: not a batch
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((2, 6))),                          # b's batch is not A's
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 5))),                          # b's height is not A's
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 6, 2))),                       # two right-hand sides
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 6)), loss="cauchy"),           # no such loss
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 6)), weights=z(4)),            # the weights' length is not m
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 6)), weights=z((2, 6))),       # their batch is not A's
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 6)), x0=z((3, 6))),            # x0's length is not n
        lambda: qr.lstsq_robust_batched(z((3, 6, 4)), z((3, 6)), scale=z(2)),              # scale's batch is not A's
        lambda: qr.lstsq_weighted_batched(z((6, 4)), z((3, 6)), z(6)),
        lambda: qr.lstsq_weighted_batched(z((3, 6, 4)), z((3, 6)), z(5)),
    ]
    for f in bad:
        with pytest.raises(qr.QRError) as ei:
            f()
        assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_robust_batched(z((3, 3, 4)), z((3, 3)))                                   # m < n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
