"""CPU-side checks of the batched damped least squares (mi355x_qr.h section 8f): declared, exported, bound, wired into the build, and
every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAMPED_API = ("qr_damped_batched_dev", "qr_gels_damped_batched_dev", "qr_gels_damped_wide_batched_dev",
              "qr_lsacc_batched_solve_damped_dev", "qr_lstsq_damped_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(DAMPED_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(DAMPED_API) <= exported
    for name in DAMPED_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8f. Batched damped" in txt and txt.index("8f. Batched damped") > txt.index("8e. Batched minimum-norm")
    for meth in ("damped_batched", "gels_damped_batched", "gels_damped_wide_batched"):
        assert callable(getattr(qr.Plan, meth))
    assert callable(qr.LsAccumulatorBatched.solve_damped) and callable(qr.lstsq_damped_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bd_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_damped_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_damped_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_damped.c" in mk and "qr_batched_damped" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bd_solve", "qrd_bd_fused", "qrd_bd_wave_route"):
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


def _ptrs():
    buf = (C.c_double * 16)()
    ibuf = (C.c_int * 4)()
    return buf, C.cast(buf, C.c_void_p), ibuf, C.cast(ibuf, C.c_void_p)     # never dereferenced


def test_solve_from_factors_rejects_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG

    def call(plan=P, R=d, n=8, ldr=8, sr=64, Z=d, nrhs=3, ldz=8, sz=24, rss=None, jp=None, sj=0, D=None, sd=0, lam=d, nlam=2, sl=2, flip=0,
             X=d, ldx=8, sx=48, xn=d, rs=d, info=di, batch=3):
        return qr.lib.qr_damped_batched_dev(plan, R, n, ldr, sr, Z, nrhs, ldz, sz, rss, jp, sj, D, sd, lam, nlam, sl, flip, X, ldx, sx, xn, rs,
                                            info, batch)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(R=None) == E and call(Z=None) == E and call(lam=None) == E and call(X=None) == E
    assert call(info=None) == E
    assert call(xn=None, rs=None, batch=0) == 0                                 # both norms are optional
    assert call(n=0) == E and call(nrhs=0) == E and call(nrhs=-1) == E and call(nlam=0) == E and call(nlam=-1) == E
    assert call(n=40, ldr=40, sr=1600, nrhs=25, ldz=40, sz=1000, ldx=40, sx=2000) == E                 # n + nrhs = 65
    assert call(n=40, ldr=40, sr=1600, nrhs=24, ldz=40, sz=960, ldx=40, sx=1920, batch=0) == 0        # 64
    assert call(n=65, ldr=65, sr=65 * 65, nrhs=1, ldz=65, sz=65, ldx=65, sx=130) == E
    assert call(ldr=7) == E and call(ldz=7) == E and call(ldx=7) == E
    assert call(sr=63) == E and call(sz=23) == E and call(sx=47) == E          # a stride between 1 and block - 1
    assert call(sr=1) == E and call(sx=8) == E
    assert call(ldr=9, sr=71) == E and call(ldr=9, sr=72, batch=0) == 0
    # lambda and D: shared (stride 0) or at least the block
    assert call(sl=0, batch=0) == 0 and call(sl=1) == E and call(sl=-1) == E and call(sl=3, batch=0) == 0
    assert call(D=d, sd=0, batch=0) == 0 and call(D=d, sd=8, batch=0) == 0 and call(D=d, sd=7) == E and call(D=d, sd=1) == E
    assert call(jp=di, sj=8, batch=0) == 0 and call(jp=di, sj=7) == E and call(jp=di, sj=0) == E
    # flip takes neither D nor jpvt
    assert call(flip=1, batch=0) == 0 and call(flip=1, D=d) == E and call(flip=1, jp=di, sj=8) == E
    assert call(batch=-1) == E and call(batch=0, R=None) == E                   # the checks come before the early return
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_tall_call_rejects_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG

    def call(plan=P, A=d, m=20, n=8, lda=20, sa=160, tau=d, st=8, B=d, nrhs=3, ldb=20, sb=60, D=None, sd=0, lam=d, nlam=2, sl=2, X=d, ldx=8,
             sx=48, xn=None, rs=None, info=di, batch=3):
        return qr.lib.qr_gels_damped_batched_dev(plan, A, m, n, lda, sa, tau, st, B, nrhs, ldb, sb, D, sd, lam, nlam, sl, X, ldx, sx, xn, rs, info,
                                                 batch)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(A=None) == E and call(tau=None) == E and call(B=None) == E and call(lam=None) == E
    assert call(X=None) == E and call(info=None) == E
    assert call(m=7) == E                                                       # m < n: the wide call's business
    assert call(m=8, lda=8, sa=64, ldb=8, sb=24, batch=0) == 0                  # square is tall
    assert call(n=0) == E and call(nrhs=0) == E and call(nlam=0) == E
    assert call(lda=19) == E and call(ldb=19) == E and call(ldx=7) == E
    assert call(sa=159) == E and call(st=7) == E and call(sb=59) == E and call(sx=47) == E and call(sb=1) == E
    assert call(sl=1) == E and call(sl=0, batch=0) == 0 and call(D=d, sd=7) == E and call(D=d, sd=0, batch=0) == 0
    assert call(m=64, n=40, lda=64, sa=64 * 40, st=40, nrhs=25, ldb=64, sb=64 * 25, ldx=40, sx=2000) == E      # Z has to ride along
    assert call(m=300, n=64, lda=300, sa=300 * 64, st=64, ldb=300, sb=900, ldx=64, sx=384) == E        # gels_batched's limits
    assert call(m=300, n=40, lda=300, sa=300 * 40, st=40, ldb=300, sb=900, ldx=40, sx=240, batch=0) == 0
    assert call(m=513, n=8, lda=513, sa=513 * 8, ldb=513, sb=513 * 3) == E
    assert call(batch=-1) == E and call(batch=0, A=None) == E
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_wide_call_and_host_twin_reject_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG

    def wide(plan=P, A=d, m=6, n=20, lda=6, sa=120, F=d, ldf=20, sf=120, tau=d, st=6, B=d, nrhs=2, ldb=6, sb=12, lam=d, nlam=3, sl=3, X=d,
             ldx=20, sx=120, xn=None, rs=None, info=di, batch=3):
        return qr.lib.qr_gels_damped_wide_batched_dev(plan, A, m, n, lda, sa, F, ldf, sf, tau, st, B, nrhs, ldb, sb, lam, nlam, sl, X, ldx, sx,
                                                      xn, rs, info, batch)

    def shaped(m, n, nrhs=1, **kw):
        return wide(m=m, n=n, lda=m, sa=m * n, ldf=n, sf=n * m, st=m, nrhs=nrhs, ldb=m, sb=m * nrhs, ldx=n, sx=3 * n * nrhs, **kw)

    assert wide(batch=0) == 0
    assert wide(plan=None) == E and wide(A=None) == E and wide(F=None) == E and wide(tau=None) == E and wide(B=None) == E
    assert wide(lam=None) == E and wide(X=None) == E and wide(info=None) == E
    assert shaped(21, 20) == E and shaped(20, 20) == E                          # m >= n: the tall call's business
    assert wide(m=0) == E and wide(nrhs=0) == E and wide(nlam=0) == E
    assert wide(lda=5) == E and wide(sa=119) == E and wide(ldf=19) == E and wide(sf=119) == E and wide(st=5) == E
    assert wide(ldb=5) == E and wide(sb=11) == E
    assert wide(ldx=19) == E and wide(sx=119) == E                              # X is n rows tall, nlam * nrhs columns wide
    assert wide(sl=2) == E and wide(sl=0, batch=0) == 0
    assert shaped(65, 300) == E and shaped(64, 256, nrhs=1) == E               # m + nrhs = 65
    assert shaped(63, 256, batch=0) == 0 and shaped(40, 300, batch=0) == 0 and shaped(8, 513) == E
    assert shaped(32, 64, nrhs=33) == E and shaped(32, 64, nrhs=32, batch=0) == 0
    assert wide(batch=-1) == E and wide(batch=0, F=None) == E

    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p, m=5, n=3, B=p, nrhs=1, batch=2, D=p, lam=p, nlam=2, X=p, xn=None, rs=None, info=inf):
        return qr.lib.qr_lstsq_damped_batched(A, m, n, B, nrhs, batch, D, lam, nlam, X, xn, rs, info)

    assert twin(batch=0) == 0 and twin(D=None, batch=0) == 0
    assert twin(A=None) == E and twin(B=None) == E and twin(lam=None) == E and twin(X=None) == E and twin(info=None) == E
    assert twin(m=0) == E and twin(n=0) == E and twin(nrhs=0) == E and twin(nlam=0) == E and twin(batch=-1) == E
    assert twin(m=3, n=5) == E and twin(m=3, n=5, D=None, batch=0) == 0        # wide: D must be NULL
    assert twin(m=300, n=64) == E and twin(m=64, n=40, nrhs=25) == E and twin(m=65, n=300, D=None) == E
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_accumulator_call_rejects_bad_arguments_without_a_device(qr):
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG
    f = qr.lib.qr_lsacc_batched_solve_damped_dev
    assert f(None, None, 0, d, 1, 1, d, 8, 8, None, None, di) == E
    fp = _plan()
    acc = C.c_void_p()
    assert qr.lib.qr_lsacc_batched_create(C.byref(acc), C.cast(C.pointer(fp), C.c_void_p), 8, 2, 0) == 0      # batch 0: no device
    try:
        def call(D=None, sd=0, lam=d, nlam=3, sl=3, X=d, ldx=8, sx=48, info=di):
            return f(acc, D, sd, lam, nlam, sl, X, ldx, sx, None, None, info)

        assert call() == 0
        assert call(lam=None) == E and call(X=None) == E and call(info=None) == E and call(nlam=0) == E
        assert call(sl=2) == E and call(sl=0) == 0 and call(D=d, sd=7) == E and call(D=d, sd=0) == 0
        assert call(ldx=7) == E and call(sx=47) == E
    finally:
        assert qr.lib.qr_lsacc_batched_destroy(acc) == 0


def test_python_wrapper_raises_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_damped_batched(np.zeros((6, 3)), np.zeros((3, 6, 1)), [0.1])               # A 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_damped_batched(np.zeros((3, 6, 3)), np.zeros((2, 6, 1)), [0.1])            # B's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_damped_batched(np.zeros((3, 6, 3)), np.zeros((3, 6, 1)), np.zeros((2, 4)))  # lam's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_damped_batched(np.zeros((3, 6, 3)), np.zeros((3, 6, 1)), [0.1], D=np.ones(4))
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_damped_batched(np.zeros((3, 3, 6)), np.zeros((3, 3, 1)), [0.1], D=np.ones(6))   # wide with D: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
