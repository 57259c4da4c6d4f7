"""CPU-side checks of the row-removal interface (mi355x_qr.h section 6b): declared, exported, bound, and argument errors without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOWNDATE_API = ("qr_tphqrt_dev", "qr_tphmqrt_dev", "qr_lsacc_pop_dev", "qr_lsacc_slide_dev", "qr_lstsq_rolling")


def test_header_declares_and_library_exports_the_row_removal(qr):
    declared = set(qr.exported_symbols())
    assert set(DOWNDATE_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(DOWNDATE_API) <= exported
    for name in DOWNDATE_API:
        f = getattr(qr.lib, name)
        assert f.argtypes, name
    txt = open(qr.HEADER).read()
    assert "6b. Row removal" in txt
    assert "NOT backward stable" in txt                    # the stability statement belongs to the interface
    for meth in ("tphqrt", "tphmqrt"):
        assert callable(getattr(qr.Plan, meth))
    for meth in ("pop", "slide"):
        assert callable(getattr(qr.LsAccumulator, meth))
    assert callable(qr.lstsq_rolling)


def test_notpd_status_is_defined_and_named(qr):
    txt = open(qr.HEADER).read()
    assert "#define QR_E_NOTPD    (-109)" in txt and qr.QR_E_NOTPD == -109
    s = qr.strerror(qr.QR_E_NOTPD)
    assert "positive-definite" in s and s != qr.strerror(-9999)


def test_host_code_stays_out_of_the_stubbed_translation_unit(qr):
    """qr_host.c is compiled against the stub device layer by the sanitizer builds: the new launch wrappers must not be called from it.
    The kernels of this interface are the signed instances in qr_update.hip: no file of their own, and the library has their launchers."""
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_th_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_downdate_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_downdate_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_downdate.c" in mk
    hipsrc = mk.split("HIPSRC =")[1].splitlines()[0].split()
    assert "qr_update" in hipsrc
    assert "qr_downdate" not in hipsrc
    assert not os.path.exists(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_downdate.hip"))
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"qrd_th_panel", "qrd_th_apply", "qrd_th_colssq"} <= exported


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h): m, n, nb, ib, ldv, ldt.  Every call below must reject its
    arguments from these alone, before it reaches a device."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


class _FakeAcc(C.Structure):
    """the leading fields of struct qr_lsacc: the plan, n, nrhs, the rows held"""
    _fields_ = [("p", C.c_void_p), ("n", C.c_int), ("nrhs", C.c_int), ("rows", C.c_longlong), ("rest", C.c_char * 256)]


def _plan(m=1000, n=300, nb=128):
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = m, n, nb, 32, (m + 127) // 128 * 128, nb
    return fp


def test_device_entry_points_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced: every call below fails its argument check first
    E = qr.QR_E_ARG
    PM = qr.tpqrt_max_rows()
    info = C.c_int(-5)

    def tphqrt(plan=P, R=d, n=300, ldr=300, B=d, pa=30, pd=10, ldb=40, T=d, ldt=32, inf=None):
        return L.qr_tphqrt_dev(plan, R, n, ldr, B, pa, pd, ldb, T, ldt, inf)

    assert tphqrt(plan=None) == E
    assert tphqrt(R=None) == E and tphqrt(B=None) == E and tphqrt(T=None) == E
    assert tphqrt(n=0) == E and tphqrt(n=301, ldr=301) == E                # above the plan's width
    assert tphqrt(pa=0, pd=0) == E
    assert tphqrt(pa=PM, pd=1, ldb=PM + 1) == E and tphqrt(pa=0, pd=PM + 1, ldb=PM + 1) == E and tphqrt(pa=PM + 1, pd=0, ldb=PM + 1) == E
    assert tphqrt(pa=2 ** 31 - 1, pd=2, ldb=2 ** 31 - 1) == E              # a sum that would wrap
    assert tphqrt(pa=-1, pd=41) == E and tphqrt(pa=41, pd=-1) == E
    assert tphqrt(ldr=299) == E and tphqrt(ldb=39) == E and tphqrt(ldt=31) == E
    assert tphqrt(n=0, inf=C.byref(info)) == E and info.value == -5         # info is written by a call that ran, not by a rejected one

    def tphmqrt(plan=P, V=d, pa=30, pd=10, n=300, ldv=40, T=d, ldt=32, C1=d, ldc1=300, C2=d, ldc2=40, nrhs=2):
        return L.qr_tphmqrt_dev(plan, V, pa, pd, n, ldv, T, ldt, C1, ldc1, C2, ldc2, nrhs)

    assert tphmqrt(plan=None) == E
    assert tphmqrt(V=None) == E and tphmqrt(T=None) == E and tphmqrt(C1=None) == E and tphmqrt(C2=None) == E
    assert tphmqrt(n=0) == E and tphmqrt(n=301, ldc1=301) == E
    assert tphmqrt(pa=0, pd=0) == E and tphmqrt(pa=PM, pd=1, ldv=PM + 1, ldc2=PM + 1) == E
    assert tphmqrt(pa=-1, pd=41) == E and tphmqrt(pa=41, pd=-1) == E
    assert tphmqrt(ldv=39) == E and tphmqrt(ldt=31) == E and tphmqrt(ldc1=299) == E and tphmqrt(ldc2=39) == E
    assert tphmqrt(nrhs=0) == E

    fa = _FakeAcc()
    fa.p, fa.n, fa.nrhs, fa.rows = P.value, 48, 2, 100
    A = C.cast(C.pointer(fa), C.c_void_p)

    def pop(acc=A, dA=d, p=10, lda=10, dB=d, ldb=10):
        return L.qr_lsacc_pop_dev(acc, dA, p, lda, dB, ldb)

    assert pop(acc=None) == E and pop(dA=None) == E and pop(dB=None) == E
    assert pop(p=0) == E and pop(p=-3) == E and pop(lda=9) == E and pop(ldb=9) == E
    assert pop(p=101, lda=101, ldb=101) == E                               # more rows than the accumulator holds

    def slide(acc=A, An=d, pn=8, ldan=8, Bn=d, ldbn=8, Ao=d, po=6, ldao=6, Bo=d, ldbo=6):
        return L.qr_lsacc_slide_dev(acc, An, pn, ldan, Bn, ldbn, Ao, po, ldao, Bo, ldbo)

    assert slide(acc=None) == E and slide(An=None) == E and slide(Bn=None) == E and slide(Ao=None) == E and slide(Bo=None) == E
    assert slide(pn=0) == E and slide(po=0) == E and slide(pn=-1) == E and slide(po=-1) == E
    assert slide(ldan=7) == E and slide(ldbn=7) == E and slide(ldao=5) == E and slide(ldbo=5) == E
    assert slide(po=101, ldao=101, ldbo=101) == E
    assert fa.rows == 100


def test_removals_that_leave_fewer_rows_than_columns_are_refused_without_a_device(qr):
    """no triangle of full rank can remain: QR_E_NOTPD from the host's bookkeeping alone (removing every row is the extreme case)"""
    L = qr.lib
    fp = _plan()
    fa = _FakeAcc()
    fa.p, fa.n, fa.nrhs, fa.rows = C.addressof(fp), 48, 1, 60
    A = C.cast(C.pointer(fa), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)
    assert L.qr_lsacc_pop_dev(A, d, 60, 60, d, 60) == qr.QR_E_NOTPD
    assert L.qr_lsacc_pop_dev(A, d, 13, 13, d, 13) == qr.QR_E_NOTPD
    assert L.qr_lsacc_slide_dev(A, d, 1, 1, d, 1, d, 14, 14, d, 14) == qr.QR_E_NOTPD
    assert fa.rows == 60


def test_lstsq_rolling_rejects_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    L = qr.lib
    E = qr.QR_E_ARG

    def call(A=p, m=16, n=4, lda=16, B=p, nrhs=1, ldb=16, window=8, step=2, X=p, resid=None):
        return L.qr_lstsq_rolling(A, m, n, lda, B, nrhs, ldb, window, step, X, resid)

    assert call(A=None) == E and call(B=None) == E and call(X=None) == E
    assert call(n=0) == E and call(m=0) == E and call(nrhs=0) == E
    assert call(window=3) == E                                             # window < n
    assert call(step=0) == E and call(step=-2) == E and call(step=9) == E  # step < 1, step > window
    assert call(window=17) == E                                            # window > m
    assert call(lda=15) == E and call(ldb=15) == E
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_rolling(np.zeros((16, 4)), np.zeros(16), 8, 0)
    assert ei.value.status == E
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_rolling(np.zeros((16, 4)), np.zeros(15), 8, 2)            # B's height is not A's
    assert ei.value.status == E
