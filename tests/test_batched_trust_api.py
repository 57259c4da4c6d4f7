"""CPU-side checks of the batched trust-region step (mi355x_qr.h section 8g): declared, exported, bound, wired into the build, and every
argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUST_API = ("qr_trust_batched_dev", "qr_gels_trust_batched_dev", "qr_gels_trust_wide_batched_dev", "qr_lsacc_batched_solve_trust_dev",
             "qr_lstsq_trust_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(TRUST_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(TRUST_API) <= exported
    for name in TRUST_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8g. Batched trust-region" in txt and txt.index("8g. Batched trust-region") > txt.index("8f. Batched damped")
    assert "Out of scope: a trust-region search" not in txt                   # 8f no longer lists it as missing
    for meth in ("trust_batched", "gels_trust_batched", "gels_trust_wide_batched"):
        assert callable(getattr(qr.Plan, meth))
    assert callable(qr.LsAccumulatorBatched.solve_trust) and callable(qr.lstsq_trust_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bt_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_trust_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_trust_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_trust.c" in mk and "qr_batched_trust" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bt_solve", "qrd_bt_fused", "qrd_bt_args"):
        assert w in dev
    # one elimination for both files: the damped kernels and the search call the same device functions
    hdr = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_batched_dev.h")).read()
    for fn in ("bd_wave_elim", "bd_wg_elim"):
        assert fn + "(" in hdr
        for f in ("qr_batched_damped.hip", "qr_batched_trust.hip"):
            assert fn in open(os.path.join(ROOT, "cuda-qr_amd", "csrc", f)).read(), (fn, f)


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


NAN = float("nan")


def test_solve_from_factors_rejects_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG

    def call(plan=P, R=d, n=8, ldr=8, sr=64, Z=d, ldz=8, sz=8, rss=None, jp=None, sj=0, D=None, sd=0, delta=d, sdel=1, lam0=None, sl0=0,
             rtol=0.1, maxit=10, flip=0, X=d, ldx=8, sx=8, lam=d, xn=d, rs=d, it=di, st=di, info=di, batch=3):
        return qr.lib.qr_trust_batched_dev(plan, R, n, ldr, sr, Z, ldz, sz, rss, jp, sj, D, sd, delta, sdel, lam0, sl0, rtol, maxit, flip, X, ldx,
                                           sx, lam, xn, rs, it, st, info, batch)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(R=None) == E and call(Z=None) == E and call(delta=None) == E and call(X=None) == E
    assert call(lam=None) == E and call(info=None) == E
    assert call(xn=None, rs=None, it=None, st=None, batch=0) == 0               # the norms, iter and status are optional
    assert call(n=0) == E and call(n=-1) == E
    assert call(n=64, ldr=64, sr=4096, ldz=64, sz=64, ldx=64, sx=64) == E      # the right-hand side is the 65th column
    assert call(n=63, ldr=63, sr=63 * 63, ldz=63, sz=63, ldx=63, sx=63, batch=0) == 0
    assert call(rtol=0.0) == E and call(rtol=1.0) == E and call(rtol=-0.1) == E and call(rtol=NAN) == E and call(rtol=1e-6, batch=0) == 0
    assert call(maxit=0) == E and call(maxit=-1) == E and call(maxit=1, batch=0) == 0
    assert call(ldr=7) == E and call(ldz=7) == E and call(ldx=7) == E
    assert call(sr=63) == E and call(sz=7) == E and call(sx=7) == E and call(sr=1) == E and call(sx=0) == E
    assert call(ldr=9, sr=71) == E and call(ldr=9, sr=72, batch=0) == 0
    # delta, lam0 and D: shared (stride 0) or at least the block
    assert call(sdel=0, batch=0) == 0 and call(sdel=-1) == E and call(sdel=5, batch=0) == 0
    assert call(lam0=d, sl0=0, batch=0) == 0 and call(lam0=d, sl0=1, batch=0) == 0 and call(lam0=d, sl0=-1) == E
    assert call(lam0=None, sl0=-1, batch=0) == 0                                 # no starting guess: its stride is not looked at
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

    def call(plan=P, A=d, m=20, n=8, lda=20, sa=160, tau=d, st=8, B=d, ldb=20, sb=20, D=None, sd=0, delta=d, sdel=1, lam0=None, sl0=0, rtol=0.1,
             maxit=10, X=d, ldx=8, sx=8, lam=d, info=di, batch=3):
        return qr.lib.qr_gels_trust_batched_dev(plan, A, m, n, lda, sa, tau, st, B, ldb, sb, D, sd, delta, sdel, lam0, sl0, rtol, maxit, X, ldx, sx,
                                                lam, None, None, None, None, info, batch)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(A=None) == E and call(tau=None) == E and call(B=None) == E and call(delta=None) == E
    assert call(X=None) == E and call(lam=None) == E and call(info=None) == E
    assert call(m=7) == E                                                       # m < n: the wide call's business
    assert call(m=8, lda=8, sa=64, ldb=8, sb=8, batch=0) == 0                   # square is tall
    assert call(n=0) == E and call(rtol=0.0) == E and call(rtol=1.5) == E and call(maxit=0) == E
    assert call(lda=19) == E and call(ldb=19) == E and call(ldx=7) == E
    assert call(sa=159) == E and call(st=7) == E and call(sb=19) == E and call(sx=7) == E and call(sb=1) == E
    assert call(sdel=-1) == E and call(sdel=0, batch=0) == 0 and call(D=d, sd=7) == E and call(D=d, sd=0, batch=0) == 0
    assert call(m=300, n=64, lda=300, sa=300 * 64, st=64, ldb=300, sb=300, ldx=64, sx=64) == E         # b has to ride along
    assert call(m=300, n=40, lda=300, sa=300 * 40, st=40, ldb=300, sb=300, ldx=40, sx=40, batch=0) == 0
    assert call(m=513, n=8, lda=513, sa=513 * 8, ldb=513, sb=513) == E          # gels_batched's limits
    assert call(batch=-1) == E and call(batch=0, A=None) == E
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_wide_call_and_host_twin_reject_bad_arguments_without_a_device(qr):
    fp = _plan()
    P = C.cast(C.pointer(fp), C.c_void_p)
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG

    def wide(plan=P, A=d, m=6, n=20, lda=6, sa=120, F=d, ldf=20, sf=120, tau=d, st=6, B=d, ldb=6, sb=6, delta=d, sdel=1, lam0=None, sl0=0,
             rtol=0.1, maxit=10, X=d, ldx=20, sx=20, lam=d, info=di, batch=3):
        return qr.lib.qr_gels_trust_wide_batched_dev(plan, A, m, n, lda, sa, F, ldf, sf, tau, st, B, ldb, sb, delta, sdel, lam0, sl0, rtol, maxit,
                                                     X, ldx, sx, lam, None, None, None, None, info, batch)

    def shaped(m, n, **kw):
        return wide(m=m, n=n, lda=m, sa=m * n, ldf=n, sf=n * m, st=m, ldb=m, sb=m, ldx=n, sx=n, **kw)

    assert wide(batch=0) == 0
    assert wide(plan=None) == E and wide(A=None) == E and wide(F=None) == E and wide(tau=None) == E and wide(B=None) == E
    assert wide(delta=None) == E and wide(X=None) == E and wide(lam=None) == E and wide(info=None) == E
    assert shaped(21, 20) == E and shaped(20, 20) == E                          # m >= n: the tall call's business
    assert wide(m=0) == E and wide(rtol=0.0) == E and wide(rtol=1.0) == E and wide(maxit=0) == E
    assert wide(lda=5) == E and wide(sa=119) == E and wide(ldf=19) == E and wide(sf=119) == E and wide(st=5) == E
    assert wide(ldb=5) == E and wide(sb=5) == E
    assert wide(ldx=19) == E and wide(sx=19) == E                               # X is n rows tall
    assert wide(sdel=-1) == E and wide(sdel=0, batch=0) == 0 and wide(lam0=d, sl0=-1) == E
    assert shaped(64, 256) == E and shaped(63, 256, batch=0) == 0 and shaped(40, 300, batch=0) == 0 and shaped(8, 513) == E
    assert wide(batch=-1) == E and wide(batch=0, F=None) == E

    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p, m=5, n=3, b=p, batch=2, D=p, delta=p, lam0=None, rtol=0.1, maxit=10, X=p, lam=p, info=inf):
        return qr.lib.qr_lstsq_trust_batched(A, m, n, b, batch, D, delta, lam0, rtol, maxit, X, lam, None, None, None, None, info)

    assert twin(batch=0) == 0 and twin(D=None, batch=0) == 0 and twin(lam0=p, batch=0) == 0
    assert twin(A=None) == E and twin(b=None) == E and twin(delta=None) == E and twin(X=None) == E and twin(lam=None) == E
    assert twin(info=None) == E
    assert twin(m=0) == E and twin(n=0) == E and twin(batch=-1) == E and twin(rtol=0.0) == E and twin(rtol=1.0) == E and twin(maxit=0) == E
    assert twin(m=3, n=5) == E and twin(m=3, n=5, D=None, batch=0) == 0        # wide: D must be NULL
    assert twin(m=300, n=64) == E and twin(m=64, n=256, D=None) == E and twin(m=513, n=8) == E
    assert list(ibuf) == [0, 0, 0, 0] and not any(buf)


def test_accumulator_call_rejects_bad_arguments_without_a_device(qr):
    buf, d, ibuf, di = _ptrs()
    E = qr.QR_E_ARG
    f = qr.lib.qr_lsacc_batched_solve_trust_dev
    assert f(None, None, 0, d, 1, None, 0, 0.1, 10, d, 8, 8, d, None, None, None, None, di) == E
    fp = _plan()
    for nrhs, ok in ((1, 0), (2, E)):                                           # one right-hand side per member
        acc = C.c_void_p()
        assert qr.lib.qr_lsacc_batched_create(C.byref(acc), C.cast(C.pointer(fp), C.c_void_p), 8, nrhs, 0) == 0      # batch 0: no device
        try:
            def call(D=None, sd=0, delta=d, sdel=1, lam0=None, sl0=0, rtol=0.1, maxit=10, X=d, ldx=8, sx=8, lam=d, info=di):
                return f(acc, D, sd, delta, sdel, lam0, sl0, rtol, maxit, X, ldx, sx, lam, None, None, None, None, info)

            assert call() == ok
            if nrhs == 1:
                assert call(delta=None) == E and call(X=None) == E and call(lam=None) == E and call(info=None) == E
                assert call(rtol=0.0) == E and call(rtol=1.0) == E and call(maxit=0) == E
                assert call(sdel=-1) == E and call(sdel=0) == 0 and call(lam0=d, sl0=-1) == E and call(lam0=d, sl0=0) == 0
                assert call(D=d, sd=7) == E and call(D=d, sd=0) == 0 and call(ldx=7) == E and call(sx=7) == E
        finally:
            assert qr.lib.qr_lsacc_batched_destroy(acc) == 0


def test_python_wrapper_raises_on_bad_shapes(qr):
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_trust_batched(np.zeros((6, 3)), np.zeros((3, 6)), 1.0)                      # A 2-D: not a batch
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_trust_batched(np.zeros((3, 6, 3)), np.zeros((2, 6)), 1.0)                   # b's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_trust_batched(np.zeros((3, 6, 3)), np.zeros((3, 6, 2)), 1.0)                # two right-hand sides
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_trust_batched(np.zeros((3, 6, 3)), np.zeros((3, 6)), np.ones(2))            # delta's batch is not A's
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError) as ei:
        qr.lstsq_trust_batched(np.zeros((3, 6, 3)), np.zeros((3, 6)), 1.0, D=np.ones(4))
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_trust_batched(np.zeros((3, 3, 6)), np.zeros((3, 3)), 1.0, D=np.ones(6))     # wide with D: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.lstsq_trust_batched(np.zeros((3, 6, 3)), np.zeros((3, 6)), 1.0, rtol=1.0)
