"""CPU-side checks of the row-append interface (mi355x_qr.h section 6): declared, exported, bound, and argument errors without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPDATE_API = ("qr_tpqrt_max_rows", "qr_tpqrt_dev", "qr_tpmqrt_dev", "qr_lsacc_create", "qr_lsacc_push_dev", "qr_lsacc_rows",
              "qr_lsacc_factor_dev", "qr_lsacc_solve_dev", "qr_lsacc_reset", "qr_lsacc_destroy", "qr_lstsq_chunked")


def test_header_declares_and_library_exports_the_row_append_update(qr):
    declared = set(qr.exported_symbols())
    assert set(UPDATE_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(UPDATE_API) <= exported
    for name in UPDATE_API:
        assert hasattr(qr.lib, name), name
        f = getattr(qr.lib, name)
        assert f.argtypes is not None and (f.argtypes or name == "qr_tpqrt_max_rows"), name
    txt = open(qr.HEADER).read()
    assert "6. Row-append updating and streaming least squares" in txt
    for meth in ("tpqrt", "tpmqrt"):
        assert callable(getattr(qr.Plan, meth))
    for meth in ("push", "rows", "factor", "solve", "reset", "close"):
        assert callable(getattr(qr.LsAccumulator, meth))
    assert callable(qr.lstsq_chunked) and callable(qr.tpqrt_max_rows)


def test_row_limit_and_panel_width_are_the_documented_constants(qr):
    P = qr.tpqrt_max_rows()
    assert P in (256, 512)
    txt = open(qr.HEADER).read()
    assert f"qr_tpqrt_max_rows() = {P}" in txt
    assert "#define QR_TPQRT_PANEL 32" in txt and qr.TPQRT_PANEL == 32


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    """qr_host.c is compiled against the stub device layer by the sanitizer builds: the new launch wrappers must not be called from it"""
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_tp" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_update_c.o" in mk and "build/lab/qr_update_c.o" in mk
    assert "csrc/qr_update.c" in mk and "qr_update" in mk.split("HIPSRC =")[1].splitlines()[0]


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
    PM = qr.tpqrt_max_rows()

    def tpqrt(plan=P, R=d, n=300, ldr=300, B=d, p=40, ldb=40, T=d, ldt=32):
        return L.qr_tpqrt_dev(plan, R, n, ldr, B, p, ldb, T, ldt)

    assert tpqrt(plan=None) == E
    assert tpqrt(R=None) == E and tpqrt(B=None) == E and tpqrt(T=None) == E
    assert tpqrt(n=0) == E and tpqrt(n=301, ldr=301) == E                 # above the plan's width
    assert tpqrt(p=0) == E and tpqrt(p=PM + 1, ldb=PM + 1) == E
    assert tpqrt(ldr=299) == E and tpqrt(ldb=39) == E and tpqrt(ldt=31) == E

    def tpmqrt(plan=P, trans=b"T", V=d, p=40, n=300, ldv=40, T=d, ldt=32, C1=d, ldc1=300, C2=d, ldc2=40, nrhs=2):
        return L.qr_tpmqrt_dev(plan, trans, V, p, n, ldv, T, ldt, C1, ldc1, C2, ldc2, nrhs)

    assert tpmqrt(plan=None) == E
    assert tpmqrt(V=None) == E and tpmqrt(T=None) == E and tpmqrt(C1=None) == E and tpmqrt(C2=None) == E
    assert tpmqrt(trans=b"X") == E and tpmqrt(trans=b"C") == E
    assert tpmqrt(n=0) == E and tpmqrt(n=301, ldc1=301) == E
    assert tpmqrt(p=0) == E and tpmqrt(p=PM + 1, ldv=PM + 1, ldc2=PM + 1) == E
    assert tpmqrt(ldv=39) == E and tpmqrt(ldt=31) == E and tpmqrt(ldc1=299) == E and tpmqrt(ldc2=39) == E
    assert tpmqrt(nrhs=0) == E

    h = C.c_void_p()
    assert L.qr_lsacc_create(None, P, 300, 1) == E
    assert L.qr_lsacc_create(C.byref(h), None, 300, 1) == E
    assert L.qr_lsacc_create(C.byref(h), P, 0, 1) == E
    assert L.qr_lsacc_create(C.byref(h), P, 301, 1) == E                  # above the plan's width
    assert L.qr_lsacc_create(C.byref(h), P, 300, 0) == E
    assert h.value is None
    rows = C.c_longlong()
    assert L.qr_lsacc_push_dev(None, d, 10, 10, d, 10) == E
    assert L.qr_lsacc_rows(None, C.byref(rows)) == E
    assert L.qr_lsacc_factor_dev(None, None, None, None, None) == E
    assert L.qr_lsacc_solve_dev(None, d, 300, None) == E
    assert L.qr_lsacc_reset(None) == E and L.qr_lsacc_destroy(None) == E


def test_lstsq_chunked_rejects_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    L = qr.lib
    E = qr.QR_E_ARG

    def call(A=p, m=8, n=4, lda=8, B=p, nrhs=1, ldb=8, chunk=3, X=p, resid=None):
        return L.qr_lstsq_chunked(A, m, n, lda, B, nrhs, ldb, chunk, X, resid)

    assert call(A=None) == E and call(B=None) == E and call(X=None) == E
    assert call(n=0) == E and call(m=0) == E and call(nrhs=0) == E
    assert call(chunk=0) == E and call(chunk=-5) == E
    assert call(lda=7) == E and call(ldb=7) == E
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_chunked(np.zeros((5, 3)), np.zeros(5), 0)
    assert ei.value.status == E
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_chunked(np.zeros((5, 3)), np.zeros(4), 2)        # B's height is not A's
    assert ei.value.status == E
