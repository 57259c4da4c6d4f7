"""CPU-side checks of the pivoting interface (mi355x_qr.h section 4): declared, exported, argument errors without a device, and the
sanitizer build of the host layer still links against its stub device layer (the pivoted factorisation's launch wrappers are called
from qr_pivot.c only, which that build leaves out)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIVOT_API = ("qr_geqp3_dev", "qr_rank_dev", "qr_gelsp_dev", "qr_lstsq_pivoted")


def test_header_declares_and_library_exports_the_pivoting_api(qr):
    declared = set(qr.exported_symbols())
    assert set(PIVOT_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(PIVOT_API) <= exported
    assert "Column pivoting and rank" in open(qr.HEADER).read()


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
    rk = C.c_int(-5)
    E = qr.QR_E_ARG

    def geqp3(plan=P, A=d, m=1000, n=300, lda=1000, jp=d, tau=d):
        return L.qr_geqp3_dev(plan, A, m, n, lda, jp, tau)

    assert geqp3(plan=None) == E
    assert geqp3(A=None) == E and geqp3(jp=None) == E and geqp3(tau=None) == E
    assert geqp3(m=200) == E and geqp3(n=0) == E and geqp3(lda=999) == E
    assert geqp3(m=1001, lda=1001) == E and geqp3(n=301) == E

    def rank(plan=P, A=d, m=1000, n=300, lda=1000, rcond=-1.0, r=C.byref(rk)):
        return L.qr_rank_dev(plan, A, m, n, lda, rcond, r)

    assert rank(plan=None) == E
    assert rank(A=None) == E and rank(r=None) == E
    assert rank(m=200) == E and rank(n=0) == E and rank(lda=999) == E and rank(m=1001, lda=1001) == E and rank(n=301) == E
    assert rk.value == -5

    def gelsp(plan=P, A=d, m=1000, n=300, lda=1000, jp=d, tau=d, B=d, nrhs=1, ldb=1000, rcond=-1.0, res=None, r=None):
        return L.qr_gelsp_dev(plan, A, m, n, lda, jp, tau, B, nrhs, ldb, rcond, res, r)

    assert gelsp(plan=None) == E
    assert gelsp(A=None) == E and gelsp(jp=None) == E and gelsp(tau=None) == E and gelsp(B=None) == E
    assert gelsp(m=200) == E and gelsp(n=0) == E and gelsp(nrhs=0) == E and gelsp(lda=999) == E and gelsp(ldb=999) == E
    assert gelsp(m=1001, lda=1001, ldb=1001) == E and gelsp(n=301) == E
    assert gelsp(m=200, res=d, r=C.byref(rk)) == E and rk.value == -5


def test_lstsq_pivoted_rejects_bad_arguments_without_a_device(qr):
    dp = C.POINTER(C.c_double)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    L = qr.lib
    E = qr.QR_E_ARG
    assert L.qr_lstsq_pivoted(None, 8, 4, p, 1, -1.0, p, p, None, None) == E
    assert L.qr_lstsq_pivoted(p, 8, 4, None, 1, -1.0, p, p, None, None) == E
    assert L.qr_lstsq_pivoted(p, 8, 4, p, 1, -1.0, None, p, None, None) == E
    assert L.qr_lstsq_pivoted(p, 3, 4, p, 1, -1.0, p, p, None, None) == E         # m < n
    assert L.qr_lstsq_pivoted(p, 8, 0, p, 1, -1.0, p, p, None, None) == E
    assert L.qr_lstsq_pivoted(p, 8, 4, p, 0, -1.0, p, None, None, None) == E
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_pivoted(np.zeros((3, 5)), np.zeros(3))
    assert ei.value.status == E
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_pivoted(np.zeros((6, 5)), np.zeros(4))         # B's height is not A's
    assert ei.value.status == E
    with pytest.raises(qr.QRError) as ei:
        qr.qr_pivoted(np.zeros((3, 5)))
    assert ei.value.status == E


def test_python_wrappers_report_a_missing_device_or_an_argument_error(qr):
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(qr.QRError, match="no HIP device"):
            qr.lstsq_pivoted(np.ones((6, 3)), np.ones(6))
    fp = _plan()
    pl = qr.Plan(1000, 300, borrowed=C.addressof(fp))
    for call in (lambda: pl.geqp3(1, 200, 300, 1000, 1, 1), lambda: pl.rank(1, 1000, 301, 1000),
                 lambda: pl.gelsp(1, 1000, 300, 1000, 1, 1, 1, 0, 1000)):
        with pytest.raises(qr.QRError) as ei:
            call()
        assert ei.value.status == qr.QR_E_ARG


def test_host_layer_sanitizer_build_still_links_without_the_pivoted_factorisation():
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355XQR_")}
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "cuda-qr_amd"), "asan"], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    assert "host layer sanitize run ok" in out.stdout
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_pivot_" not in src
