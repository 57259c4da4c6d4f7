"""CPU-side checks of the batched equality-constrained least squares (mi355x_qr.h section 8h): declared, exported, bound, wired into the
build, and every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSE_API = ("qr_gglse_batched_max_rows", "qr_gglse_batched_dev", "qr_lstsq_constrained_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(LSE_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(LSE_API) <= exported
    for name in LSE_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8h. Batched equality-constrained least squares" in txt
    assert txt.index("8h. Batched equality-constrained") > txt.index("8g. Batched trust-region")
    assert callable(qr.Plan.gglse_batched) and callable(qr.gglse_batched_max_rows) and callable(qr.lstsq_constrained_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bl_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_lse_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_lse_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_lse.c" in mk and "qr_batched_lse" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bl_solve", "qrd_bl_max_rows", "qrd_bl_wave_route"):
        assert w in dev


def test_max_rows_at_its_edges(qr):
    mr = qr.gglse_batched_max_rows
    assert mr(8, 2, 1) == 512 and mr(31, 7, 1) == 512
    assert mr(63, 1, 1) > 0 and mr(63, 1, 2) == 0             # n + nrhs = 64 is taken, 65 is not
    assert mr(64, 1, 1) == 0 and mr(32, 8, 33) == 0
    assert mr(8, 9, 1) == 0 and mr(8, 0, 1) == 0 and mr(8, -1, 1) == 0          # p > n, p < 1
    assert mr(0, 1, 1) == 0 and mr(8, 2, 0) == 0
    assert mr(8, 8, 1) == 512                                                    # p == n
    # the budget: (n + nrhs) qb_ld(m) + p qb_ld(n) + nrhs (n + p) + 72 doubles within 160 KiB, qb_ld(x) the smallest value >= x that is 2 mod 32
    def ld(x):
        return ((x + 29) // 32) * 32 + 2

    for n, p, nrhs in ((63, 20, 1), (63, 63, 1), (40, 12, 2), (33, 10, 31), (48, 1, 16)):
        m = mr(n, p, nrhs)
        small = p * ld(n) + nrhs * (n + p) + 72
        assert 1 <= m <= 512
        assert 8 * ((n + nrhs) * ld(m) + small) <= 160 * 1024
        assert m == 512 or 8 * ((n + nrhs) * ld(m + 1) + small) > 160 * 1024
    assert mr(63, 16, 1) >= 256 and mr(63, 20, 1) >= 130                          # the shapes of the tests and the measurement fit


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

    def call(plan=P, A=d, m=20, n=8, lda=20, sa=160, Cm=d, p=3, ldc=3, sc=24, B=d, ldb=20, sb=40, D=d, ldd=3, sd=6, nrhs=2, X=d, ldx=8, sx=16,
             Lm=d, ldl=3, sl=6, res=d, sres=2, info=di, batch=3):
        return L.qr_gglse_batched_dev(plan, A, m, n, lda, sa, Cm, p, ldc, sc, B, ldb, sb, D, ldd, sd, nrhs, X, ldx, sx, Lm, ldl, sl, res, sres,
                                      info, batch)

    def shaped(m, n, p, nrhs=1, **kw):
        return call(m=m, n=n, lda=m, sa=m * n, p=p, ldc=p, sc=p * n, ldb=m, sb=m * nrhs, ldd=p, sd=p * nrhs, nrhs=nrhs, ldx=n, sx=n * nrhs,
                    ldl=p, sl=p * nrhs, sres=nrhs, **kw)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(A=None) == E and call(Cm=None) == E and call(B=None) == E and call(D=None) == E
    assert call(X=None) == E and call(info=None) == E
    assert call(Lm=None, ldl=0, sl=0, batch=0) == 0 and call(res=None, sres=0, batch=0) == 0          # the optional outputs
    assert call(n=0) == E and shaped(70, 65, 3) == E and shaped(70, 64, 3) == E
    assert call(p=0) == E and call(p=-1) == E and shaped(20, 8, 9) == E                                # p < 1, p > n
    assert call(m=0) == E and call(m=-1) == E
    assert shaped(4, 8, 3) == E and shaped(5, 8, 3, batch=0) == 0                                       # m + p < n; m == n - p is taken
    assert shaped(1, 8, 8, batch=0) == 0                                                                # p == n with a single row of A
    assert call(nrhs=0) == E and call(nrhs=-1) == E
    assert shaped(70, 40, 3, nrhs=25) == E and shaped(70, 40, 3, nrhs=24, batch=0) == 0                 # n + nrhs > 64
    mr = L.qr_gglse_batched_max_rows(63, 20, 1)
    assert 0 < mr < 512 and shaped(mr, 63, 20, batch=0) == 0 and shaped(mr + 1, 63, 20) == E            # m above the rows that are held
    assert shaped(512, 8, 3, batch=0) == 0 and shaped(513, 8, 3) == E
    assert call(lda=19) == E and call(ldc=2) == E and call(ldb=19) == E and call(ldd=2) == E and call(ldx=7) == E and call(ldl=2) == E
    assert call(sa=159) == E and call(sc=23) == E and call(sb=39) == E and call(sd=5) == E and call(sx=15) == E and call(sl=5) == E
    assert call(sres=1) == E
    assert call(lda=21, sa=167) == E and call(lda=21, sa=168, batch=0) == 0
    assert call(batch=-1) == E
    assert call(batch=0, A=None) == E and call(batch=0, ldx=7) == E                                     # the checks come before the early return
    assert list(ibuf) == [0, 0, 0, 0]


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p_ = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p_, m=5, n=3, Cm=p_, p=2, b=p_, d=p_, nrhs=1, batch=2, X=p_, Lm=p_, res=p_, info=inf):
        return L.qr_lstsq_constrained_batched(A, m, n, Cm, p, b, d, nrhs, batch, X, Lm, res, info)

    assert twin(batch=0) == 0 and twin(batch=0, Lm=None, res=None) == 0
    assert twin(A=None) == E and twin(Cm=None) == E and twin(b=None) == E and twin(d=None) == E and twin(X=None) == E and twin(info=None) == E
    assert twin(p=0) == E and twin(p=4) == E and twin(m=0) == E and twin(n=0) == E and twin(nrhs=0) == E and twin(batch=-1) == E
    assert twin(m=1, n=4, p=2) == E and twin(m=2, n=4, p=2, batch=0) == 0
    assert twin(n=40, p=3, m=50, nrhs=25) == E and twin(m=513, batch=0) == E
    assert list(inf) == [0] * 16


def test_python_wrapper_raises_on_bad_shapes(qr):
    z = np.zeros
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((6, 4)), z((3, 2, 4)), z((3, 6, 1)), z((3, 2, 1)))              # A 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((3, 6, 4)), z((2, 2, 4)), z((3, 6, 1)), z((3, 2, 1)))           # C's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((3, 6, 4)), z((3, 2, 4)), z((2, 6, 1)), z((3, 2, 1)))           # b's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((3, 6, 4)), z((3, 2, 5)), z((3, 6, 1)), z((3, 2, 1)))           # C's width is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((3, 6, 4)), z((3, 2, 4)), z((3, 5, 1)), z((3, 2, 1)))           # b's height is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((3, 6, 4)), z((3, 2, 4)), z((3, 6, 1)), z((3, 3, 1)))           # d's height is not C's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_constrained_batched(z((3, 6, 4)), z((3, 2, 4)), z((3, 6, 2)), z((3, 2, 1)))           # d's right-hand sides are not b's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_constrained_batched(z((3, 1, 4)), z((3, 2, 4)), z((3, 1, 1)), z((3, 2, 1)))           # m + p < n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
