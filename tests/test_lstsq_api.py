"""CPU-side checks of the least-squares interface (mi355x_qr.h section 3): declared, exported, argument errors without a device,
and the sanitizer build of the host layer still links against its stub device layer (the solve's launch wrappers live in
qr_solve.c, which that build leaves out)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_API = ("qr_build_t_dev", "qr_ormqr_dev", "qr_solve_r_dev", "qr_gels_dev", "qr_lstsq")


def test_header_declares_and_library_exports_the_solve(qr):
    declared = set(qr.exported_symbols())
    assert set(SOLVE_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(SOLVE_API) <= exported
    txt = open(qr.HEADER).read()
    assert "#define QR_E_SINGULAR (-107)" in txt
    assert "Solving with the factors" in txt


def test_singular_status_has_its_own_text(qr):
    assert qr.QR_E_SINGULAR == -107
    s = qr.strerror(qr.QR_E_SINGULAR)
    assert "zero diagonal" in s
    assert s not in (qr.strerror(qr.QR_E_ARG), qr.strerror(-104), qr.strerror(-7))


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

    def ormqr(plan=P, tr=b"T", A=d, m=1000, n=300, lda=1000, tau=d, T=None, ldt=0, Cm=d, nrhs=1, ldc=1000):
        return L.qr_ormqr_dev(plan, tr, A, m, n, lda, tau, T, ldt, Cm, nrhs, ldc)

    assert ormqr(plan=None) == E
    assert ormqr(tr=b"X") == E
    assert ormqr(A=None) == E and ormqr(tau=None) == E and ormqr(Cm=None) == E
    assert ormqr(m=200, n=300, lda=1000, ldc=1000) == E          # m < n
    assert ormqr(nrhs=0) == E
    assert ormqr(lda=999) == E and ormqr(ldc=999) == E
    assert ormqr(m=1001, lda=1001, ldc=1001) == E                 # above the plan's height
    assert ormqr(n=301) == E                                       # above the plan's width
    assert ormqr(T=d, ldt=127) == E                                # ldt < the plan's nb
    assert ormqr(n=0) == E

    def build_t(plan=P, A=d, m=1000, n=300, lda=1000, tau=d, T=d, ldt=128):
        return L.qr_build_t_dev(plan, A, m, n, lda, tau, T, ldt)

    assert build_t(plan=None) == E
    assert build_t(T=None) == E and build_t(A=None) == E and build_t(tau=None) == E
    assert build_t(ldt=64) == E and build_t(lda=10) == E and build_t(m=100) == E and build_t(n=400) == E

    def solve_r(plan=P, A=d, n=300, lda=1000, B=d, nrhs=1, ldb=300):
        return L.qr_solve_r_dev(plan, A, n, lda, B, nrhs, ldb)

    assert solve_r(plan=None) == E
    assert solve_r(A=None) == E and solve_r(B=None) == E
    assert solve_r(n=0) == E and solve_r(n=301, ldb=400) == E
    assert solve_r(lda=299) == E and solve_r(ldb=299) == E and solve_r(nrhs=0) == E

    def gels(plan=P, A=d, m=1000, n=300, lda=1000, tau=d, B=d, nrhs=1, ldb=1000):
        return L.qr_gels_dev(plan, A, m, n, lda, tau, B, nrhs, ldb)

    assert gels(plan=None) == E
    assert gels(A=None) == E and gels(tau=None) == E and gels(B=None) == E
    assert gels(m=200) == E and gels(nrhs=0) == E and gels(ldb=999) == E and gels(lda=999) == E
    assert gels(m=1001, lda=1001, ldb=1001) == E and gels(n=301) == E


def test_lstsq_rejects_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    L = qr.lib
    E = qr.QR_E_ARG
    assert L.qr_lstsq(None, 8, 4, p, 1, p, p) == E
    assert L.qr_lstsq(p, 8, 4, None, 1, p, p) == E
    assert L.qr_lstsq(p, 8, 4, p, 1, None, p) == E
    assert L.qr_lstsq(p, 3, 4, p, 1, p, p) == E         # m < n
    assert L.qr_lstsq(p, 8, 0, p, 1, p, p) == E
    assert L.qr_lstsq(p, 8, 4, p, 0, p, None) == E
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq(np.zeros((3, 5)), np.zeros(3))
    assert ei.value.status == E
    with pytest.raises(qr.QRError):
        qr.lstsq(np.zeros((6, 5)), np.zeros(4))         # B's height is not A's


def test_host_layer_sanitizer_build_still_links_without_the_solve():
    """qr_host.c must call no launch wrapper that the stub device layer (tests/c/qrd_stub.c) lacks: the solve's live in qr_solve.c"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355XQR_")}
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-qr_amd"), "asan"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    assert "host layer sanitize run ok" in out.stdout
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    for fn in ("qrd_ormqr_skinny", "qrd_trsm_step"):
        assert fn not in src
