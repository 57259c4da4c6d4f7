"""CPU-side checks of the batched pivoted interface (mi355x_qr.h section 8b): declared, exported, bound, and argument errors without a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIVOT_API = ("qr_geqp3_batched_dev", "qr_rank_batched_dev", "qr_gelsp_batched_dev", "qr_gelsy_batched_dev", "qr_thin_pivoted_batched",
             "qr_lstsq_pivoted_batched")


def test_header_declares_and_library_exports_the_pivoted_batched_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(PIVOT_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(PIVOT_API) <= exported
    for name in PIVOT_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8b." in txt and "8. Batched" in txt
    assert "#define QR_BATCHED_MAX_N 64" in txt
    for meth in ("geqp3_batched", "rank_batched", "gelsp_batched", "gelsy_batched"):
        assert callable(getattr(qr.Plan, meth))
    assert callable(qr.qr_pivoted_batched) and callable(qr.lstsq_pivoted_batched)


def test_launch_wrappers_stay_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_b_" not in src
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_b_geqp3", "qrd_b_rank", "qrd_b_solve_piv"):
        assert w in dev


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h), smaller than the calls' shapes: the batched calls are not bound by
    it.  Every call below must reject its arguments before it reaches a device."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def test_device_entry_points_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced: every call below fails its argument check first (or has batch == 0)
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    def geqp3(plan=P, A=d, m=100, n=20, lda=100, sa=2000, jp=di, sj=20, tau=d, st=20, batch=3):
        return L.qr_geqp3_batched_dev(plan, A, m, n, lda, sa, jp, sj, tau, st, batch)

    assert geqp3(plan=None) == E and geqp3(A=None) == E and geqp3(jp=None) == E and geqp3(tau=None) == E
    assert geqp3(m=19) == E                                                  # m < n
    assert geqp3(n=0) == E and geqp3(n=-1) == E
    assert geqp3(m=100, n=65, sa=6500, sj=65, st=65) == E                    # n > QR_BATCHED_MAX_N
    assert geqp3(m=513, lda=513, sa=513 * 20) == E                           # m > 512 at 20 columns
    assert geqp3(m=300, n=64, lda=300, sa=300 * 64, sj=64, st=64) == E       # 64 columns of 300 rows do not fit
    assert geqp3(m=483, n=40, lda=483, sa=483 * 40, sj=40, st=40) == E       # 40 * 514 + 72 doubles do not fit either
    assert geqp3(m=482, n=40, lda=482, sa=482 * 40, sj=40, st=40, batch=0) == 0
    assert geqp3(m=290, n=64, lda=290, sa=290 * 64, sj=64, st=64, batch=0) == 0
    assert geqp3(lda=99) == E
    assert geqp3(sa=1999) == E and geqp3(lda=101, sa=2019) == E              # strideA < lda * n
    assert geqp3(sj=19) == E and geqp3(st=19) == E
    assert geqp3(batch=-1) == E
    assert geqp3(batch=0) == 0
    assert geqp3(batch=0, jp=None) == E                                      # the checks come before the early return

    def rank(plan=P, A=d, m=100, n=20, lda=100, sa=2000, rcond=-1.0, out=di, batch=3):
        return L.qr_rank_batched_dev(plan, A, m, n, lda, sa, rcond, out, batch)

    assert rank(plan=None) == E and rank(A=None) == E and rank(out=None) == E
    assert rank(m=19) == E and rank(n=0) == E and rank(n=65, sa=6500) == E
    assert rank(m=513, lda=513, sa=513 * 20) == E and rank(m=300, n=64, lda=300, sa=300 * 64) == E
    assert rank(m=483, n=40, lda=483, sa=483 * 40) == E
    assert rank(lda=99) == E and rank(sa=1999) == E and rank(batch=-1) == E
    assert rank(rcond=float("nan")) == E
    assert rank(batch=0) == 0 and rank(batch=0, rcond=0.25) == 0
    assert rank(m=482, n=40, lda=482, sa=482 * 40, batch=0) == 0 and rank(m=290, n=64, lda=290, sa=290 * 64, batch=0) == 0

    for fn in (L.qr_gelsp_batched_dev, L.qr_gelsy_batched_dev):
        def gelsx(plan=P, A=d, m=100, n=20, lda=100, sa=2000, jp=di, sj=20, tau=d, st=20, B=d, nrhs=2, ldb=100, sb=200, rcond=-1.0,
                  res=d, rk=di, batch=3):
            return fn(plan, A, m, n, lda, sa, jp, sj, tau, st, B, nrhs, ldb, sb, rcond, res, rk, batch)

        assert gelsx(plan=None) == E and gelsx(A=None) == E and gelsx(jp=None) == E and gelsx(tau=None) == E and gelsx(B=None) == E
        assert gelsx(m=19) == E and gelsx(n=0) == E and gelsx(n=65, sa=6500, sj=65, st=65) == E
        assert gelsx(m=513, lda=513, sa=513 * 20, ldb=513, sb=513 * 2) == E
        assert gelsx(m=300, n=64, lda=300, sa=300 * 64, sj=64, st=64, ldb=300, sb=600) == E
        assert gelsx(m=483, n=40, lda=483, sa=483 * 40, sj=40, st=40, ldb=483, sb=966) == E
        assert gelsx(lda=99) == E and gelsx(ldb=99) == E and gelsx(nrhs=0) == E and gelsx(nrhs=-2) == E
        assert gelsx(sa=1999) == E and gelsx(sj=19) == E and gelsx(st=19) == E and gelsx(sb=199) == E
        assert gelsx(batch=-1) == E and gelsx(rcond=float("nan")) == E
        assert gelsx(batch=0) == 0 and gelsx(batch=0, nrhs=300, sb=30000) == 0
        assert gelsx(batch=0, res=None, rk=None) == 0                        # dresid and drank are optional
        assert gelsx(m=482, n=40, lda=482, sa=482 * 40, sj=40, st=40, ldb=482, sb=964, batch=0) == 0
        assert gelsx(m=290, n=64, lda=290, sa=290 * 64, sj=64, st=64, ldb=290, sb=580, batch=0) == 0
        assert gelsx(batch=0, B=None) == E
    assert list(ibuf) == [0, 0, 0, 0]


def test_host_twins_reject_bad_arguments_without_a_device(qr):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    jb = (C.c_int * 16)()
    j = C.cast(jb, ip)
    L = qr.lib
    E = qr.QR_E_ARG

    def thin(A=p, m=8, n=4, batch=2, Q=p, R=p, jp=j):
        return L.qr_thin_pivoted_batched(A, m, n, batch, Q, R, jp)

    assert thin(A=None) == E and thin(Q=None) == E and thin(R=None) == E and thin(jp=None) == E
    assert thin(m=3) == E and thin(n=0) == E and thin(batch=-1) == E
    assert thin(m=600, n=4) == E and thin(m=70, n=65) == E
    assert thin(batch=0) == 0

    def lstsq(A=p, m=8, n=4, B=p, nrhs=1, batch=2, rcond=-1.0, minnorm=1, X=p, resid=None, rank=None, jp=None):
        return L.qr_lstsq_pivoted_batched(A, m, n, B, nrhs, batch, rcond, minnorm, X, resid, rank, jp)

    assert lstsq(A=None) == E and lstsq(B=None) == E and lstsq(X=None) == E
    assert lstsq(m=3) == E and lstsq(n=0) == E and lstsq(nrhs=0) == E and lstsq(batch=-1) == E
    assert lstsq(m=600, n=4) == E
    assert lstsq(batch=0) == 0 and lstsq(batch=0, minnorm=0, resid=p, rank=j, jp=j) == 0


def test_python_wrappers_raise_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.qr_pivoted_batched(np.zeros((8, 4)))                              # 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_pivoted_batched(np.zeros((8, 4)), np.zeros((3, 8, 1)))
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_pivoted_batched(np.zeros((3, 8, 4)), np.zeros((8, 1)))      # B 2-D
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_pivoted_batched(np.zeros((3, 8, 4)), np.zeros((2, 8, 1)))   # B's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_pivoted_batched(np.zeros((3, 8, 4)), np.zeros((3, 7, 1)))   # B's height is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.qr_pivoted_batched(np.zeros((2, 3, 4)))                           # m < n: rejected by the library, before any device
    assert ei.value.status == qr.QR_E_ARG
