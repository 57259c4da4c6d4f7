"""CPU-side checks of the batched SVD's interface (mi355x_qr.h section 8c): declared, exported, bound, and argument errors without a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVD_API = ("qr_gesvd_batched_dev", "qr_svd_batched")


def test_header_declares_and_library_exports_the_batched_svd(qr):
    declared = set(qr.exported_symbols())
    assert set(SVD_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(SVD_API) <= exported
    for name in SVD_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8c." in txt and "8b." in txt
    assert callable(qr.Plan.gesvd_batched) and callable(qr.svd_batched)


def test_launch_wrapper_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_b_" not in src
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    assert "qrd_b_jsvd" in dev
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "qr_batched_svd" in mk


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h), smaller than the calls' shapes: the batched calls are not bound by
    it.  Every call below must reject its arguments before it reaches a device."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def test_device_entry_point_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced: every call below fails its argument check first (or has batch == 0)
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    def svd(plan=P, ju=b"U", jv=b"V", A=d, m=100, n=20, lda=100, sa=2000, jp=di, sj=20, tau=d, st=20, S=d, ss=20, U=d, ldu=100, su=2000,
            V=d, ldv=20, sv=400, rk=di, sw=di, info=di, batch=3):
        return L.qr_gesvd_batched_dev(plan, ju, jv, A, m, n, lda, sa, jp, sj, tau, st, S, ss, U, ldu, su, V, ldv, sv, rk, sw, info, batch)

    def shape(m, n, **kw):
        return svd(m=m, n=n, lda=m, sa=m * n, sj=n, st=n, ss=n, ldu=m, su=m * n, ldv=n, sv=n * n, **kw)

    # what section 8b rejects
    assert svd(plan=None) == E and svd(A=None) == E and svd(jp=None) == E and svd(tau=None) == E
    assert svd(m=19) == E                                                    # m < n
    assert svd(n=0) == E and svd(n=-1) == E
    assert shape(100, 65) == E                                               # n > QR_BATCHED_MAX_N
    assert shape(513, 20) == E                                               # m > 512 at 20 columns
    assert shape(300, 64) == E                                               # 64 columns of 300 rows do not fit
    assert shape(483, 40) == E                                               # 40 * 514 + 72 doubles do not fit either
    assert shape(482, 40, batch=0) == 0 and shape(290, 64, batch=0) == 0
    assert shape(513, 20, batch=0) == E and shape(300, 64, batch=0) == E and shape(483, 40, batch=0) == E
    assert svd(lda=99) == E
    assert svd(sa=1999) == E and svd(lda=101, sa=2019) == E                  # strideA < lda * n
    assert svd(sj=19) == E and svd(st=19) == E
    assert svd(batch=-1) == E
    # what this section adds
    assert svd(ju=b"A") == E and svd(ju=b"V") == E and svd(ju=b"u") == E and svd(jv=b"U") == E and svd(jv=b"T") == E and svd(jv=b"\0") == E
    assert svd(S=None) == E and svd(info=None) == E
    assert svd(ss=19) == E
    assert svd(U=None) == E and svd(ldu=99) == E and svd(su=1999) == E and svd(ldu=101, su=2019) == E
    assert svd(V=None) == E and svd(ldv=19) == E and svd(sv=399) == E and svd(ldv=21, sv=419) == E
    # batch == 0 returns 0, after the checks
    assert svd(batch=0) == 0
    assert svd(batch=0, rk=None, sw=None) == 0                               # drank and dsweeps are optional
    assert svd(batch=0, ju=b"N", U=None, ldu=0, su=0) == 0                   # an output that is not wanted is not checked
    assert svd(batch=0, jv=b"N", V=None, ldv=0, sv=0) == 0
    assert svd(batch=0, ju=b"N", jv=b"N", U=None, V=None, ldu=-5, su=-1, ldv=-5, sv=-1) == 0
    assert svd(batch=0, U=None) == E and svd(batch=0, V=None) == E           # ... and one that is wanted is
    assert svd(batch=0, ju=b"X") == E and svd(batch=0, S=None) == E and svd(batch=0, info=None) == E and svd(batch=0, ss=19) == E
    assert svd(batch=0, ldu=99) == E and svd(batch=0, sv=399) == E and svd(batch=0, jp=None) == E
    assert list(ibuf) == [0, 0, 0, 0] and list(buf) == [0.0] * 16


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    a = (C.c_double * 64)()
    p = C.cast(a, dp)
    jb = (C.c_int * 16)()
    j = C.cast(jb, ip)
    L = qr.lib
    E = qr.QR_E_ARG

    def svd(A=p, m=8, n=4, batch=2, S=p, U=p, V=p, rank=j):
        return L.qr_svd_batched(A, m, n, batch, S, U, V, rank)

    assert svd(A=None) == E and svd(S=None) == E
    assert svd(m=3) == E and svd(n=0) == E and svd(batch=-1) == E            # m < n
    assert svd(m=600, n=4) == E and svd(m=70, n=65) == E and svd(m=300, n=64) == E
    assert svd(batch=0) == 0 and svd(batch=0, U=None, V=None, rank=None) == 0
    assert svd(batch=0, S=None) == E


def test_python_wrapper_raises_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.svd_batched(np.zeros((8, 4)))                                     # 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.svd_batched(np.zeros((2, 3, 4)))                                  # m < n: rejected by the library, before any device
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.svd_batched(np.zeros((2, 70, 65)), compute_uv=False)              # n > 64
    assert ei.value.status == qr.QR_E_ARG
    U, S, V, rank = qr.svd_batched(np.zeros((0, 8, 4)))                      # an empty batch: nothing is launched
    assert U.shape == (0, 8, 4) and S.shape == (0, 4) and V.shape == (0, 4, 4) and rank.shape == (0,)
