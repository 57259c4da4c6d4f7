"""CPU-side checks of the batched inequality-constrained least squares (mi355x_qr.h section 8l): declared, exported, bound, wired into the
build, the row limit against its byte formula, and every argument error without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import batched_lsei_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSEI_API = ("qr_lsei_batched_max_rows", "qr_lsei_batched_dev", "qr_lstsq_inequality_batched")


def test_header_declares_and_library_exports_the_calls(qr):
    declared = set(qr.exported_symbols())
    assert set(LSEI_API) <= declared
    out = subprocess.run(["nm", "-D", qr.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(LSEI_API) <= exported
    for name in LSEI_API:
        assert getattr(qr.lib, name).argtypes, name
    txt = open(qr.HEADER).read()
    assert "8l. Batched inequality-constrained least squares" in txt
    assert txt.index("8l. Batched inequality-constrained") > txt.index("8k. Batched covariance")
    assert callable(qr.Plan.lsei_batched) and callable(qr.lsei_batched_max_rows) and callable(qr.lstsq_inequality_batched)


def test_host_code_stays_out_of_the_stubbed_translation_unit():
    src = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_host.c")).read()
    assert "qrd_le_" not in src
    mk = open(os.path.join(ROOT, "cuda-qr_amd", "Makefile")).read()
    assert "build/qr_batched_lsei_c.o" in mk.split("\nOBJS =")[1].splitlines()[0]
    lab = mk.split("\nLAB_OBJS =")[1]
    assert "build/lab/qr_batched_lsei_c.o" in lab[:lab.index("$(LAB):")]
    assert "csrc/qr_batched_lsei.c" in mk and "qr_batched_lsei" in mk.split("HIPSRC =")[1].splitlines()[0].split()
    dev = open(os.path.join(ROOT, "cuda-qr_amd", "csrc", "qr_device.h")).read()
    for w in ("qrd_le_args", "qrd_le_solve", "qrd_le_max_rows", "qrd_le_wave_route"):
        assert w in dev


def test_max_rows_at_its_edges_and_against_its_byte_formula(qr):
    mr = qr.lsei_batched_max_rows
    assert mr(0, 4) == 0 and mr(-1, 4) == 0 and mr(64, 4) == 0 and mr(8, 0) == 0 and mr(8, 65) == 0 and mr(8, -1) == 0
    assert mr(1, 1) == 512 and mr(8, 64) == 512 and mr(31, 64) == 512
    assert mr(63, 64) == R.MAX_ROWS_63_64 and mr(63, 64) >= 130          # the shapes of the tests fit

    # the budget: (n + 1) ld(m) + (n + 1) ld(n) + 5 mg + 4 n + 72 doubles within 160 KiB, ld(x) the smallest value >= x that is 2 mod 32
    def ld(x):
        return ((x + 29) // 32) * 32 + 2

    def size(m, n, mg):
        return 8 * ((n + 1) * ld(m) + (n + 1) * ld(n) + 5 * mg + 4 * n + 72)

    for n in range(1, 64):
        for mg in (1, 7, 33, 64):
            m = mr(n, mg)
            assert m == R.max_rows(n, mg)
            assert 1 <= m <= 512
            assert size(m, n, mg) <= 160 * 1024
            assert m == 512 or size(m + 1, n, mg) > 160 * 1024
    assert any(mr(n, 64) < 512 for n in range(32, 64))
    assert bool(qr.lib.qrd_le_wave_route(64, 31)) and not qr.lib.qrd_le_wave_route(65, 31) and not qr.lib.qrd_le_wave_route(40, 32)
    for sh in R.SHAPES:
        assert sh[0] <= mr(sh[1], sh[2]), sh


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

    def call(plan=P, A=d, m=20, n=8, lda=20, sa=160, B=d, sb=20, G=d, mg=5, neq=2, ldg=5, sg=40, H=d, sh=5, maxit=0, rcond=0.0, X=d, sx=8,
             MU=d, smu=5, S=d, ss=5, st=di, sst=5, res=d, it=di, info=di, batch=3):
        return L.qr_lsei_batched_dev(plan, A, m, n, lda, sa, B, sb, G, mg, neq, ldg, sg, H, sh, maxit, rcond, X, sx, MU, smu, S, ss, st, sst,
                                     res, it, info, batch)

    def shaped(m, n, mg, neq, **kw):
        return call(m=m, n=n, lda=m, sa=m * n, sb=m, mg=mg, neq=neq, ldg=mg, sg=mg * n, sh=mg, sx=n, smu=mg, ss=mg, sst=mg, **kw)

    assert call(batch=0) == 0
    for name in ("plan", "A", "B", "G", "H", "X", "info"):
        assert call(**{name: None}) == E, name
    assert call(MU=None, smu=0, batch=0) == 0 and call(S=None, ss=0, batch=0) == 0 and call(st=None, sst=0, batch=0) == 0
    assert call(res=None, it=None, batch=0) == 0
    assert call(n=0) == E and call(n=-1) == E and shaped(70, 64, 4, 0) == E and shaped(70, 63, 4, 0, batch=0) == 0
    assert shaped(20, 8, 0, 0) == E and shaped(20, 8, 65, 0) == E and shaped(20, 8, 64, 0, batch=0) == 0                # 1 <= mg <= 64
    assert shaped(20, 8, 5, -1) == E and shaped(20, 8, 5, 6) == E and shaped(20, 8, 5, 5, batch=0) == 0                  # 0 <= neq <= mg
    assert shaped(20, 3, 5, 4) == E and shaped(20, 3, 5, 3, batch=0) == 0                                               # neq <= n
    assert shaped(0, 8, 9, 8) == E and shaped(1, 8, 9, 7, batch=0) == 0 and shaped(1, 8, 9, 6) == E                      # m >= 1, m + neq >= n
    assert shaped(7, 8, 5, 0) == E and shaped(8, 8, 5, 0, batch=0) == 0 and shaped(1, 1, 1, 0, batch=0) == 0
    mr = L.qr_lsei_batched_max_rows(63, 64)
    assert 0 < mr < 512 and shaped(mr, 63, 64, 0, batch=0) == 0 and shaped(mr + 1, 63, 64, 0) == E                       # m above the rows held
    assert shaped(512, 8, 5, 0, batch=0) == 0 and shaped(513, 8, 5, 0) == E
    assert call(lda=19) == E and call(sa=159) == E and call(lda=21, sa=167) == E and call(lda=21, sa=168, batch=0) == 0
    assert call(sb=19) == E and call(sx=7) == E and call(smu=4) == E and call(ss=4) == E and call(sst=4) == E
    assert call(ldg=4) == E and call(sg=39) == E and call(ldg=7, sg=55) == E and call(ldg=7, sg=56, batch=0) == 0
    assert call(sg=0, batch=0) == 0 and call(sg=-1) == E and call(sh=0, batch=0) == 0 and call(sh=4) == E and call(sh=-1) == E   # 0: shared
    assert call(maxit=-5, batch=0) == 0 and call(maxit=1, batch=0) == 0 and call(rcond=-1.0, batch=0) == 0 and call(rcond=1e-8, batch=0) == 0
    assert call(batch=-1) == E
    assert call(batch=0, A=None) == E and call(batch=0, sx=7) == E and call(batch=0, sh=3) == E                          # the checks come before the early return
    assert list(ibuf) == [0, 0, 0, 0]


def test_host_twin_rejects_bad_arguments_without_a_device(qr):
    L = qr.lib
    E = qr.QR_E_ARG
    dp = C.POINTER(C.c_double)
    hb = (C.c_double * 64)()
    p_ = C.cast(hb, dp)
    inf = (C.c_int * 16)()

    def twin(A=p_, m=5, n=3, b=p_, G=p_, mg=4, neq=1, h=p_, maxit=0, rcond=0.0, batch=2, X=p_, MU=p_, S=p_, st=inf, res=p_, it=inf, info=inf):
        return L.qr_lstsq_inequality_batched(A, m, n, b, G, mg, neq, h, maxit, rcond, batch, X, MU, S, st, res, it, info)

    assert twin(batch=0) == 0 and twin(batch=0, MU=None, S=None, st=None, res=None, it=None) == 0
    for name in ("A", "b", "G", "h", "X", "info"):
        assert twin(**{name: None}) == E, name
    assert twin(m=2, neq=0) == E and twin(n=0) == E and twin(m=70, n=64) == E and twin(batch=-1) == E
    assert twin(mg=0) == E and twin(mg=65) == E and twin(neq=-1) == E and twin(neq=5) == E and twin(neq=4) == E
    assert twin(m=513, batch=0) == E and twin(m=512, batch=0) == 0 and twin(batch=0, A=None) == E
    assert list(inf) == [0] * 16


def test_python_wrappers_raise_on_bad_shapes(qr):
    z = np.zeros
    bad = [
        lambda: qr.lstsq_inequality_batched(z((6, 4)), z((3, 6)), z((2, 4)), z(2)),                # A 2-D: not a batch
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((2, 6)), z((2, 4)), z(2)),             # b's batch is not A's
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 5)), z((2, 4)), z(2)),             # b's height is not A's
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6, 2)), z((2, 4)), z(2)),          # two right-hand sides
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6)), z((2, 5)), z(2)),             # G's width is not n
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6)), z((2, 2, 4)), z(2)),          # G's batch is not A's
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6)), z((2, 4)), z(3)),             # h's length is not mg
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6)), z((2, 4)), z((2, 2))),        # h's batch is not A's
        lambda: qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6)), z((2, 4)), None),             # no h
    ]
    for f in bad:
        with pytest.raises(qr.QRError) as ei:
            f()
        assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument") as ei:
        qr.lstsq_inequality_batched(z((3, 3, 4)), z((3, 3)), z((2, 4)), z(2))                      # m + neq < n: rejected by the library
    assert ei.value.status == qr.QR_E_ARG
    with pytest.raises(qr.QRError, match="invalid argument"):
        qr.lstsq_inequality_batched(z((3, 6, 4)), z((3, 6)), z((2, 4)), z(2), neq=3)               # neq > mg
