"""CPU-side checks of the minimum-norm interface (mi355x_qr.h section 5): declared, exported, argument errors without a device, and the
entry points of section 3 still refuse m < n."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINNORM_API = ("qr_solve_rt_dev", "qr_minnorm_dev", "qr_gels_t_dev", "qr_transpose_dev", "qr_gels_wide_dev", "qr_lstsq_minnorm")


def test_header_declares_and_library_exports_the_minimum_norm_solve(qr):
    declared = set(qr.exported_symbols())
    assert set(MINNORM_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(MINNORM_API) <= exported
    for name in MINNORM_API:
        assert hasattr(qr.lib, name) and getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "5. Minimum-norm solutions: underdetermined and transposed systems" in txt
    for meth in ("solve_rt", "minnorm", "gels_t", "transpose", "gels_wide"):
        assert callable(getattr(qr.Plan, meth))
    assert callable(qr.lstsq_minnorm)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    """qr_host.c is compiled against the stub device layer by the sanitizer builds: the new launch wrappers must not be called from it"""
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    for fn in ("qrd_trsm_t_step", "qrd_transpose_tiled"):
        assert fn not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_minnorm_c.o" in mk and "build/lab/qr_minnorm_c.o" in mk


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h): m, n, nb, ib, ldv, ldt.  Every call below must reject its
    arguments from these alone, before it reaches a device."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


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

    def solve_rt(plan=P, A=d, n=300, lda=1000, B=d, nrhs=1, ldb=300):
        return L.qr_solve_rt_dev(plan, A, n, lda, B, nrhs, ldb)

    assert solve_rt(plan=None) == E
    assert solve_rt(A=None) == E and solve_rt(B=None) == E
    assert solve_rt(n=0) == E and solve_rt(n=301, ldb=400) == E          # above the plan's width
    assert solve_rt(lda=299) == E and solve_rt(ldb=299) == E and solve_rt(nrhs=0) == E

    def minnorm(plan=P, A=d, m=1000, n=300, lda=1000, tau=d, T=None, ldt=0, B=d, nrhs=1, ldb=1000):
        return L.qr_minnorm_dev(plan, A, m, n, lda, tau, T, ldt, B, nrhs, ldb)

    assert minnorm(plan=None) == E
    assert minnorm(A=None) == E and minnorm(tau=None) == E and minnorm(B=None) == E
    assert minnorm(m=200) == E                                            # m < n
    assert minnorm(n=0) == E and minnorm(nrhs=0) == E
    assert minnorm(lda=999) == E and minnorm(ldb=999) == E
    assert minnorm(m=1001, lda=1001, ldb=1001) == E and minnorm(n=301) == E
    assert minnorm(T=d, ldt=127) == E                                     # ldt < the plan's nb

    def gels_t(plan=P, A=d, m=1000, n=300, lda=1000, tau=d, B=d, nrhs=1, ldb=1000):
        return L.qr_gels_t_dev(plan, A, m, n, lda, tau, B, nrhs, ldb)

    assert gels_t(plan=None) == E
    assert gels_t(A=None) == E and gels_t(tau=None) == E and gels_t(B=None) == E
    assert gels_t(m=200) == E                                             # m < n
    assert gels_t(nrhs=0) == E and gels_t(ldb=999) == E and gels_t(lda=999) == E and gels_t(n=0) == E
    assert gels_t(m=1001, lda=1001, ldb=1001) == E and gels_t(n=301) == E

    def transpose(plan=P, S=d, rows=40, cols=30, lds=40, D=d, ldd=30):
        return L.qr_transpose_dev(plan, S, rows, cols, lds, D, ldd)

    assert transpose(plan=None) == E
    assert transpose(S=None) == E and transpose(D=None) == E
    assert transpose(rows=0) == E and transpose(cols=0) == E
    assert transpose(lds=39) == E and transpose(ldd=29) == E

    # the wide system is m x n = 300 x 1000 on the plan for its transpose (1000 x 300)
    def gels_wide(plan=P, A=d, m=300, n=1000, lda=300, F=d, ldf=1000, tau=d, B=d, nrhs=1, ldb=1000):
        return L.qr_gels_wide_dev(plan, A, m, n, lda, F, ldf, tau, B, nrhs, ldb)

    assert gels_wide(plan=None) == E
    assert gels_wide(A=None) == E and gels_wide(F=None) == E and gels_wide(tau=None) == E and gels_wide(B=None) == E
    assert gels_wide(m=1000, n=300, lda=1000, ldf=300, ldb=300) == E      # m > n
    assert gels_wide(m=0) == E and gels_wide(nrhs=0) == E
    assert gels_wide(lda=299) == E and gels_wide(ldf=999) == E and gels_wide(ldb=999) == E
    assert gels_wide(n=1001, ldf=1001, ldb=1001) == E                     # n above the plan's rows
    assert gels_wide(m=301, lda=301) == E                                 # m above the plan's columns
    fq = _plan(300, 300)                                                  # a plan sized for the wide shape's rows, not its transpose
    Q = C.cast(C.pointer(fq), C.c_void_p)
    assert gels_wide(plan=Q) == E


def test_lstsq_minnorm_rejects_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    L = qr.lib
    E = qr.QR_E_ARG
    assert L.qr_lstsq_minnorm(None, 4, 8, p, 1, p) == E
    assert L.qr_lstsq_minnorm(p, 4, 8, None, 1, p) == E
    assert L.qr_lstsq_minnorm(p, 4, 8, p, 1, None) == E
    assert L.qr_lstsq_minnorm(p, 8, 4, p, 1, p) == E          # m > n
    assert L.qr_lstsq_minnorm(p, 0, 4, p, 1, p) == E
    assert L.qr_lstsq_minnorm(p, 4, 8, p, 0, p) == E
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_minnorm(np.zeros((5, 3)), np.zeros(5))
    assert ei.value.status == E
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_minnorm(np.zeros((3, 5)), np.zeros(4))       # B's height is not A's
    assert ei.value.status == E


def test_full_rank_least_squares_still_refuses_wide_matrices(qr):
    """section 3 keeps its behaviour: m < n is QR_E_ARG there, the wide case has entry points of its own"""
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq(np.zeros((3, 5)), np.zeros(3))
    assert ei.value.status == qr.QR_E_ARG
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)
    assert qr.lib.qr_gels_dev(P, d, 200, 300, 1000, d, d, 1, 1000) == qr.QR_E_ARG
    assert qr.lib.qr_ormqr_dev(P, b"N", d, 200, 300, 1000, d, None, 0, d, 1, 1000) == qr.QR_E_ARG
