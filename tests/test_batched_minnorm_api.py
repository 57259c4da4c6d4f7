"""CPU-side checks of the batched minimum-norm solves (mi355x_qr.h section 8e): declared, exported, bound, wired into the build, and
every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINNORM_API = ("qr_minnorm_batched_dev", "qr_gels_t_batched_dev", "qr_transpose_batched_dev", "qr_gels_wide_batched_dev",
               "qr_lstsq_minnorm_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(MINNORM_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(MINNORM_API) <= exported
    for name in MINNORM_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8e. Batched minimum-norm" in txt and txt.index("8e. Batched minimum-norm") > txt.index("8d. Batched row")
    for meth in ("minnorm_batched", "gels_t_batched", "gels_wide_batched", "transpose_batched"):
        assert callable(getattr(qr.Plan, meth))
    assert callable(qr.lstsq_minnorm_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bm_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_minnorm_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_minnorm_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_minnorm.c" in mk and "qr_batched_minnorm" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bm_fused", "qrd_bm_apply", "qrd_bm_transpose"):
        assert w in dev


class _FakePlan(C.Structure):
    """the leading fields of struct qr_plan (csrc/qr_plan_internal.h).  Every call below must reject its arguments before it reaches a
    device, or have batch == 0."""
    _fields_ = [("m", C.c_int), ("n", C.c_int), ("nb", C.c_int), ("ib", C.c_int), ("ldv", C.c_int), ("ldt", C.c_int),
                ("rest", C.c_char * 8192)]


def _plan():
    fp = _FakePlan()
    fp.m, fp.n, fp.nb, fp.ib, fp.ldv, fp.ldt = 16, 4, 4, 4, 128, 4
    return fp


def test_tall_calls_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)           # never dereferenced
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    for fn in (L.qr_minnorm_batched_dev, L.qr_gels_t_batched_dev):
        def call(plan=P, A=d, m=20, n=8, lda=20, sa=160, tau=d, st=8, B=d, nrhs=3, ldb=20, sb=60, info=di, batch=3, fn=fn):
            return fn(plan, A, m, n, lda, sa, tau, st, B, nrhs, ldb, sb, info, batch)

        assert call(batch=0) == 0
        assert call(plan=None) == E and call(A=None) == E and call(tau=None) == E and call(B=None) == E and call(info=None) == E
        assert call(m=7) == E                                                   # m < n: the wide call's business
        assert call(n=0) == E and call(n=65, m=65, lda=65, sa=65 * 65, st=65, ldb=65, sb=195) == E
        assert call(nrhs=0) == E and call(nrhs=-1) == E
        assert call(lda=19) == E and call(ldb=19) == E                          # ldb >= m: X is m rows tall
        assert call(ldb=8, sb=24) == E                                          # B alone would fit: X does not
        assert call(sa=159) == E and call(st=7) == E and call(sb=59) == E
        assert call(lda=21, sa=167) == E and call(lda=21, sa=168, batch=0) == 0
        assert call(batch=-1) == E
        assert call(batch=0, A=None) == E                                       # the checks come before the early return
        assert call(m=300, n=64, lda=300, sa=300 * 64, st=64, ldb=300, sb=900) == E          # 64 columns of 300 rows do not fit
        assert call(m=300, n=40, lda=300, sa=300 * 40, st=40, ldb=300, sb=900, batch=0) == 0
        assert call(m=513, n=8, lda=513, sa=513 * 8, ldb=513, sb=513 * 3) == E
        # n + nrhs = 65, and far more: the composed route (gels_t) / the solve alone takes any nrhs
        assert call(m=64, n=32, lda=64, sa=64 * 32, st=32, nrhs=33, ldb=64, sb=64 * 33, batch=0) == 0
        assert call(nrhs=300, sb=6000, batch=0) == 0
        assert call(m=300, n=40, lda=300, sa=300 * 40, st=40, nrhs=30, ldb=300, sb=9000, batch=0) == 0   # 70 columns do not fit: composed
    assert list(ibuf) == [0, 0, 0, 0]


def test_transpose_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)
    E = qr.QR_E_ARG

    def tr(plan=P, S=d, rows=5, cols=9, lds=5, ss=45, D=d, ldd=9, sd=45, batch=3):
        return L.qr_transpose_batched_dev(plan, S, rows, cols, lds, ss, D, ldd, sd, batch)

    assert tr(batch=0) == 0
    assert tr(plan=None) == E and tr(S=None) == E and tr(D=None) == E
    assert tr(rows=0) == E and tr(cols=0) == E and tr(rows=-1) == E
    assert tr(lds=4) == E and tr(ldd=8) == E and tr(ss=44) == E and tr(sd=44) == E
    assert tr(rows=512, cols=512, lds=512, ss=512 * 512, ldd=512, sd=512 * 512, batch=0) == 0
    assert tr(rows=513, lds=513, ss=513 * 9, sd=513 * 9) == E and tr(cols=513, ss=5 * 513, ldd=513, sd=513 * 5) == E
    assert tr(batch=-1) == E and tr(batch=0, S=None) == E


def test_wide_call_and_host_twin_reject_bad_arguments_without_a_device(qr):
    L = qr.lib
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf = (C.c_double * 16)()
    d = C.cast(buf, C.c_void_p)
    ibuf = (C.c_int * 4)()
    di = C.cast(ibuf, C.c_void_p)
    E = qr.QR_E_ARG

    def wide(plan=P, A=d, m=6, n=20, lda=6, sa=120, F=d, ldf=20, sf=120, tau=d, st=6, B=d, nrhs=2, ldb=20, sb=40, info=di, batch=3):
        return L.qr_gels_wide_batched_dev(plan, A, m, n, lda, sa, F, ldf, sf, tau, st, B, nrhs, ldb, sb, info, batch)

    def shaped(m, n, nrhs=1, **kw):
        return wide(m=m, n=n, lda=m, sa=m * n, ldf=n, sf=n * m, st=m, nrhs=nrhs, ldb=n, sb=n * nrhs, **kw)

    assert wide(batch=0) == 0
    assert wide(plan=None) == E and wide(A=None) == E and wide(F=None) == E and wide(tau=None) == E and wide(B=None) == E
    assert wide(info=None) == E
    assert shaped(21, 20) == E                                                  # m > n: the tall call's business
    assert shaped(20, 20, batch=0) == 0                                         # square is both
    assert wide(m=0) == E and wide(nrhs=0) == E and wide(nrhs=-1) == E
    assert wide(lda=5) == E and wide(sa=119) == E
    assert wide(ldf=19) == E and wide(sf=119) == E and wide(ldf=21, sf=125) == E and wide(ldf=21, sf=126, batch=0) == 0
    assert wide(st=5) == E
    assert wide(ldb=19) == E                                                    # ldb >= n: X is n rows tall
    assert wide(ldb=6, sb=12) == E                                              # B alone would fit: X does not
    assert wide(sb=39) == E
    assert wide(batch=-1) == E and wide(batch=0, F=None) == E
    # the limits: m <= 64, and n x m as section 8 describes
    assert shaped(65, 300) == E
    assert shaped(64, 256, batch=0) == 0
    assert shaped(64, 257) == E
    assert shaped(40, 300, batch=0) == 0
    assert shaped(64, 300) == E
    assert shaped(8, 512, batch=0) == 0 and shaped(8, 513) == E
    # m + nrhs = 65 at a shape that then goes composed is accepted, and so is any nrhs
    assert shaped(32, 64, nrhs=33, batch=0) == 0
    assert shaped(6, 20, nrhs=300, batch=0) == 0
    assert shaped(40, 300, nrhs=30, batch=0) == 0

    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p, m=3, n=5, B=p, nrhs=1, batch=2, X=p, info=inf):
        return L.qr_lstsq_minnorm_batched(A, m, n, B, nrhs, batch, X, info)

    assert twin(batch=0) == 0
    assert twin(A=None) == E and twin(B=None) == E and twin(X=None) == E and twin(info=None) == E
    assert twin(m=6) == E                                                       # m > n
    assert twin(m=0) == E and twin(nrhs=0) == E and twin(batch=-1) == E
    assert twin(m=65, n=300) == E and twin(m=64, n=257) == E and twin(m=64, n=256, batch=0) == 0
    assert list(ibuf) == [0, 0, 0, 0]


def test_python_wrapper_raises_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_minnorm_batched(np.zeros((6, 7)), np.zeros((3, 6, 1)))                      # A 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_minnorm_batched(np.zeros((3, 6, 7)), np.zeros((2, 6, 1)))                   # B's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_minnorm_batched(np.zeros((3, 6, 7)), np.zeros((3, 5, 1)))                   # B's height is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_minnorm_batched(np.zeros((3, 7, 6)), np.zeros((3, 7, 1)))                   # m > n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
