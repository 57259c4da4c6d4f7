"""CPU-side checks of the batched bound-constrained least squares (mi355x_qr.h section 8i): declared, exported, bound, wired into the
build, the row limit against its byte formula, and every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batched_bvls_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BVLS_API = ("qr_bvls_batched_max_rows", "qr_bvls_batched_dev", "qr_lstsq_bounded_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(BVLS_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(BVLS_API) <= exported
    for name in BVLS_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8i. Batched bound-constrained least squares" in txt
    assert txt.index("8i. Batched bound-constrained") > txt.index("8h. Batched equality-constrained")
    assert callable(qr.Plan.bvls_batched) and callable(qr.bvls_batched_max_rows) and callable(qr.lstsq_bounded_batched)
    assert callable(qr.nnls_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_bv_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_bvls_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_bvls_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_bvls.c" in mk and "qr_batched_bvls" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_bv_args", "qrd_bv_solve", "qrd_bv_max_rows", "qrd_bv_wave_route"):
        assert w in dev


def test_max_rows_at_its_edges_and_against_its_byte_formula(qr):
    mr = qr.bvls_batched_max_rows
    assert mr(0) == 0 and mr(-1) == 0 and mr(64) == 0 and mr(65) == 0
    assert mr(1) == 512 and mr(8) == 512 and mr(31) == 512
    assert mr(63) == R.MAX_ROWS_63 and mr(63) >= 256          # the shapes of the tests and the measurement fit

    # the budget: (n + 1) qb_ld(m) + 6 n + 72 doubles within 160 KiB, qb_ld(x) the smallest value >= x that is 2 mod 32
    def ld(x):
        return ((x + 29) // 32) * 32 + 2

    for n in range(1, 64):
        m = mr(n)
        assert m == R.max_rows(n)
        assert n <= m <= 512
        assert 8 * ((n + 1) * ld(m) + 6 * n + 72) <= 160 * 1024
        assert m == 512 or 8 * ((n + 1) * ld(m + 1) + 6 * n + 72) > 160 * 1024
    assert any(mr(n) < 512 for n in range(32, 64))
    assert bool(qr.lib.qrd_bv_wave_route(64, 31)) and not qr.lib.qrd_bv_wave_route(65, 31) and not qr.lib.qrd_bv_wave_route(40, 32)


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

    def call(plan=P, A=d, m=20, n=8, lda=20, sa=160, B=d, sb=20, lo=d, hi=d, sbnd=8, maxit=0, X=d, sx=8, W=d, sw=8, st=di, sst=8, res=d, it=di,
             info=di, batch=3):
        return L.qr_bvls_batched_dev(plan, A, m, n, lda, sa, B, sb, lo, hi, sbnd, maxit, X, sx, W, sw, st, sst, res, it, info, batch)

    def shaped(m, n, **kw):
        return call(m=m, n=n, lda=m, sa=m * n, sb=m, sbnd=n, sx=n, sw=n, sst=n, **kw)

    assert call(batch=0) == 0
    assert call(plan=None) == E and call(A=None) == E and call(B=None) == E and call(X=None) == E and call(info=None) == E
    assert call(lo=None, batch=0) == 0 and call(hi=None, batch=0) == 0 and call(lo=None, hi=None, batch=0) == 0         # unbounded sides
    assert call(W=None, sw=0, batch=0) == 0 and call(st=None, sst=0, batch=0) == 0 and call(res=None, it=None, batch=0) == 0
    assert call(n=0) == E and call(n=-1) == E and shaped(70, 64) == E and shaped(70, 65) == E and shaped(70, 63, batch=0) == 0
    assert shaped(7, 8) == E and shaped(8, 8, batch=0) == 0 and shaped(1, 1, batch=0) == 0                               # m < n
    mr = L.qr_bvls_batched_max_rows(63)
    assert 0 < mr < 512 and shaped(mr, 63, batch=0) == 0 and shaped(mr + 1, 63) == E                                     # m above the rows held
    assert shaped(512, 8, batch=0) == 0 and shaped(513, 8) == E
    assert call(lda=19) == E and call(sa=159) == E and call(lda=21, sa=167) == E and call(lda=21, sa=168, batch=0) == 0
    assert call(sb=19) == E and call(sx=7) == E and call(sw=7) == E and call(sst=7) == E
    assert call(sbnd=7) == E and call(sbnd=1) == E and call(sbnd=-1) == E and call(sbnd=0, batch=0) == 0 and call(sbnd=9, batch=0) == 0
    assert call(lo=None, hi=None, sbnd=7) == E and call(lo=None, hi=None, sbnd=0, batch=0) == 0                          # checked without bounds too
    assert call(maxit=-5, batch=0) == 0 and call(maxit=1, batch=0) == 0
    assert call(batch=-1) == E
    assert call(batch=0, A=None) == E and call(batch=0, sx=7) == E and call(batch=0, sbnd=3) == E                        # the checks come before the early return
    assert list(ibuf) == [0, 0, 0, 0]


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p_ = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p_, m=5, n=3, b=p_, lo=p_, hi=p_, maxit=0, batch=2, X=p_, W=p_, st=inf, res=p_, it=inf, info=inf):
        return L.qr_lstsq_bounded_batched(A, m, n, b, lo, hi, maxit, batch, X, W, st, res, it, info)

    assert twin(batch=0) == 0 and twin(batch=0, lo=None, hi=None, W=None, st=None, res=None, it=None) == 0
    assert twin(A=None) == E and twin(b=None) == E and twin(X=None) == E and twin(info=None) == E
    assert twin(m=2) == E and twin(n=0) == E and twin(m=70, n=64) == E and twin(batch=-1) == E
    assert twin(m=513, batch=0) == E and twin(m=512, batch=0) == 0 and twin(batch=0, A=None) == E
    assert list(inf) == [0] * 16


def test_python_wrappers_raise_on_bad_shapes(qr):
    z = np.zeros
    bad = [
        lambda: qr.lstsq_bounded_batched(z((6, 4)), z((3, 6))),                            # A 2-D: not a batch
        lambda: qr.lstsq_bounded_batched(z((3, 6, 4)), z((2, 6))),                         # b's batch is not A's
        lambda: qr.lstsq_bounded_batched(z((3, 6, 4)), z((3, 5))),                         # b's height is not A's
        lambda: qr.lstsq_bounded_batched(z((3, 6, 4)), z((3, 6, 2))),                      # two right-hand sides
        lambda: qr.lstsq_bounded_batched(z((3, 6, 4)), z((3, 6)), lo=z(3)),                # lo's length is not n
        lambda: qr.lstsq_bounded_batched(z((3, 6, 4)), z((3, 6)), hi=z((2, 4))),           # hi's batch is not A's
        lambda: qr.lstsq_bounded_batched(z((3, 6, 4)), z((3, 6)), lo=z((3, 4, 1))),        # lo 3-D
        lambda: qr.nnls_batched(z((6, 4)), z((3, 6))),
        lambda: qr.nnls_batched(z((3, 6, 4)), z((3, 5))),
    ]
    for f in bad:
        with pytest.raises(qr.QRError) as ei:
            f()
        assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_bounded_batched(z((3, 3, 4)), z((3, 3)))                                  # m < n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
