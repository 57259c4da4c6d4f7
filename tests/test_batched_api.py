"""CPU-side checks of the batched interface (mi355x_qr.h section 8): declared, exported, bound, and argument errors without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHED_API = ("qr_batched_max_rows", "qr_geqrf_batched_dev", "qr_ormqr_batched_dev", "qr_orgqr_batched_dev", "qr_gels_batched_dev",
               "qr_thin_batched", "qr_lstsq_batched")


def test_header_declares_and_library_exports_the_batched_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(BATCHED_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(BATCHED_API) <= exported
    for name in BATCHED_API:
        assert getattr(qr.lib, name).argtypes is not None, name
    for name in BATCHED_API[1:]:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8. Batched" in txt
    assert "#define QR_BATCHED_MAX_N 64" in txt             # the eighth symbol of the section
    for meth in ("geqrf_batched", "ormqr_batched", "orgqr_batched", "gels_batched"):
        assert callable(getattr(qr.Plan, meth))
    assert callable(qr.qr_batched) and callable(qr.lstsq_batched) and callable(qr.batched_max_rows)


def test_max_rows_table(qr):
    assert [qr.lib.qr_batched_max_rows(c) for c in (1, 32, 33, 64, 65, 0)] == [512, 512, 256, 256, 0, 0]
    assert [qr.batched_max_rows(c) for c in (1, 32, 33, 64, 65, 0)] == [512, 512, 256, 256, 0, 0]
    assert qr.lib.qr_batched_max_rows(-3) == 0


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    """qr_host.c is compiled against the stub device layer by the sanitizer builds: the new launch wrappers must not be called from it"""
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_b_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched.c" in mk and "qr_batched" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_b_geqrf", "qrd_b_ormqr", "qrd_b_eye", "qrd_b_trsm", "qrd_b_max_rows"):
        assert w in dev


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h); the plan is deliberately SMALLER than the calls' shapes: the
    batched calls are not bound by it.  Every call below must reject its arguments before it reaches a device."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


def test_device_entry_points_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced: every call below fails its argument check first (or has batch == 0)
    E = qr.QR_E_ARG

    def geqrf(plan=P, A=d, m=100, n=20, lda=100, sa=2000, tau=d, st=20, batch=3):
        return L.qr_geqrf_batched_dev(plan, A, m, n, lda, sa, tau, st, batch)

    assert geqrf(plan=None) == E and geqrf(A=None) == E and geqrf(tau=None) == E
    assert geqrf(m=19) == E                                                  # m < n
    assert geqrf(n=0) == E and geqrf(n=-1) == E
    assert geqrf(m=100, n=65, sa=6500, st=65) == E                           # n > QR_BATCHED_MAX_N
    assert geqrf(m=513, lda=513, sa=513 * 20) == E                           # m > max_rows(20) = 512
    assert geqrf(m=300, n=64, lda=300, sa=300 * 64, st=64) == E              # m > max_rows(64) = 256, and 64 columns of 300 rows do not fit
    # between the table and the LDS limit the shape itself decides: n columns at the leading dimension 2 mod 32, + 72 doubles, in 160 KiB
    assert geqrf(m=300, n=40, lda=300, sa=300 * 40, st=40, batch=0) == 0     # 40 * 322 doubles fit
    assert geqrf(m=482, n=40, lda=482, sa=482 * 40, st=40, batch=0) == 0     # 40 * 482 + 72 = 19352 <= 20480
    assert geqrf(m=483, n=40, lda=483, sa=483 * 40, st=40) == E              # 40 * 514 do not
    assert geqrf(m=290, n=64, lda=290, sa=290 * 64, st=64, batch=0) == 0 and geqrf(m=291, n=64, lda=291, sa=291 * 64, st=64) == E
    assert geqrf(m=512, n=39, lda=512, sa=512 * 39, st=39, batch=0) == 0 and geqrf(m=512, n=40, lda=512, sa=512 * 40, st=40) == E
    assert geqrf(lda=99) == E
    assert geqrf(sa=1999) == E and geqrf(lda=101, sa=2019) == E              # strideA < lda * n
    assert geqrf(st=19) == E
    assert geqrf(batch=-1) == E
    assert geqrf(batch=0) == 0
    assert geqrf(batch=0, A=None) == E                                       # the checks come before the early return

    def ormqr(plan=P, trans=b"T", A=d, m=100, n=20, lda=100, sa=2000, tau=d, st=20, Cm=d, nrhs=5, ldc=100, sc=500, batch=3):
        return L.qr_ormqr_batched_dev(plan, trans, A, m, n, lda, sa, tau, st, Cm, nrhs, ldc, sc, batch)

    assert ormqr(plan=None) == E and ormqr(A=None) == E and ormqr(tau=None) == E and ormqr(Cm=None) == E
    assert ormqr(trans=b"X") == E and ormqr(trans=b"t") == E
    assert ormqr(m=19) == E and ormqr(n=0) == E and ormqr(n=65, sa=6500, st=65) == E
    assert ormqr(m=513, lda=513, sa=513 * 20, ldc=513, sc=513 * 5) == E
    assert ormqr(lda=99) == E and ormqr(ldc=99) == E and ormqr(nrhs=0) == E
    assert ormqr(sa=1999) == E and ormqr(st=19) == E and ormqr(sc=499) == E
    assert ormqr(batch=-1) == E
    assert ormqr(batch=0) == 0 and ormqr(batch=0, trans=b"N", nrhs=70, sc=7000) == 0

    def orgqr(plan=P, A=d, m=100, n=20, lda=100, sa=2000, tau=d, st=20, Q=d, ldq=100, sq=2000, batch=3):
        return L.qr_orgqr_batched_dev(plan, A, m, n, lda, sa, tau, st, Q, ldq, sq, batch)

    assert orgqr(plan=None) == E and orgqr(A=None) == E and orgqr(tau=None) == E and orgqr(Q=None) == E
    assert orgqr(m=19) == E and orgqr(n=0) == E and orgqr(n=65, sa=6500, st=65, sq=6500) == E
    assert orgqr(m=513, lda=513, sa=513 * 20, ldq=513, sq=513 * 20) == E
    assert orgqr(lda=99) == E and orgqr(ldq=99) == E
    assert orgqr(sa=1999) == E and orgqr(st=19) == E and orgqr(sq=1999) == E
    assert orgqr(batch=-1) == E
    assert orgqr(batch=0) == 0

    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)

    def gels(plan=P, A=d, m=100, n=20, lda=100, sa=2000, tau=d, st=20, B=d, nrhs=2, ldb=100, sb=200, info=di, batch=3):
        return L.qr_gels_batched_dev(plan, A, m, n, lda, sa, tau, st, B, nrhs, ldb, sb, info, batch)

    assert gels(plan=None) == E and gels(A=None) == E and gels(tau=None) == E and gels(B=None) == E and gels(info=None) == E
    assert gels(m=19) == E and gels(n=0) == E and gels(n=65, sa=6500, st=65) == E
    assert gels(m=513, lda=513, sa=513 * 20, ldb=513, sb=513 * 2) == E
    assert gels(lda=99) == E and gels(ldb=99) == E and gels(nrhs=0) == E and gels(nrhs=-2) == E
    assert gels(sa=1999) == E and gels(st=19) == E and gels(sb=199) == E
    assert gels(batch=-1) == E
    assert gels(batch=0) == 0 and gels(batch=0, nrhs=300, sb=30000) == 0
    assert list(ibuf) == [0, 0, 0, 0]


def test_host_twins_reject_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    inf = (C.c_int * 4)()
    L = qr.lib
    E = qr.QR_E_ARG

    def thin(A=p, m=8, n=4, batch=2, Q=p, R=p):
        return L.qr_thin_batched(A, m, n, batch, Q, R)

    assert thin(A=None) == E and thin(Q=None) == E and thin(R=None) == E
    assert thin(m=3) == E and thin(n=0) == E and thin(batch=-1) == E
    assert thin(m=600, n=4) == E and thin(m=70, n=65) == E
    assert thin(batch=0) == 0

    def lstsq(A=p, m=8, n=4, B=p, nrhs=1, batch=2, X=p, resid=None, info=inf):
        return L.qr_lstsq_batched(A, m, n, B, nrhs, batch, X, resid, info)

    assert lstsq(A=None) == E and lstsq(B=None) == E and lstsq(X=None) == E and lstsq(info=None) == E
    assert lstsq(m=3) == E and lstsq(n=0) == E and lstsq(nrhs=0) == E and lstsq(batch=-1) == E
    assert lstsq(m=600, n=4) == E
    assert lstsq(batch=0) == 0


def test_python_wrappers_raise_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.qr_batched(np.zeros((8, 4)))                                      # 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_batched(np.zeros((8, 4)), np.zeros((3, 8, 1)))
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_batched(np.zeros((3, 8, 4)), np.zeros((8, 1)))              # B 2-D
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_batched(np.zeros((3, 8, 4)), np.zeros((2, 8, 1)))           # B's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_batched(np.zeros((3, 8, 4)), np.zeros((3, 7, 1)))           # B's height is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.qr_batched(np.zeros((2, 3, 4)))                                   # m < n: rejected by the library, before any device
    assert ei.value.status == qr.QR_E_ARG
